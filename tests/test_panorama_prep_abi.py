"""CPU: the panorama -> training-batch path (crop with folded rotation, area resize, tensor tonemap, PanoramaBatcher)
reaches its C ABI entry points with arguments that convert to the bound signatures -- WITHOUT a GPU.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_rasteriser_grad_abi.py``, restated here).  The
launchers' own argument validation is checked against the built library (it returns before anything touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recorder:
    def __init__(self, signatures):
        self.signatures, self.calls, self.args = signatures, [], []

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        restype, argtypes = self.signatures[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, call site passes %d" % (name, len(argtypes), len(args))
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError("%s: argument %d (%r) does not convert to %s" % (name, k, a, t.__name__)) from e
            self.calls.append(name)
            self.args.append((name, args))
            return 64 if restype is ctypes.c_size_t else 0
        return call

    def of(self, name):
        return [a for n, a in self.args if n == name]


@pytest.fixture
def recorder(monkeypatch):
    from emlight_amd import _lib

    def require(t, name, dtype=None):      # the dtype check stays, the device check goes
        if t.dtype != (dtype or torch.float32):
            raise _lib.EmlightHipError("%s must be %s" % (name, dtype or torch.float32))
        return t.contiguous()
    rec = _Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", require)
    return rec


class _FakeDeviceTensor(torch.Tensor):
    """A CPU tensor that says it lives on the device: lets a per-sample ``deg`` / ``fov_deg`` tensor through on this box."""
    @property
    def is_cuda(self):
        return True


def _dev(values):
    return torch.tensor(values, dtype=torch.float32).as_subclass(_FakeDeviceTensor)


# eml_pano_crop_f32(pano, is_u8, B, H, W, h, w, ratio, fov_deg, fov_dev, deg, deg_dev, out, stream)
def test_crop_scalar_arguments_go_by_value_on_the_batch_shared_path(recorder):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    out = PanoramaHandler.crop_panorama(torch.rand(3, 64, 128, 3), 60, 24, "4:3", deg=77.3)
    assert out.shape == (3, 3, 24, 32) and out.dtype == torch.float32
    (a,) = recorder.of("eml_pano_crop_f32")
    assert a[1:7] == (0, 3, 64, 128, 24, 32) and a[7] == 4 / 3
    assert a[8] == 60.0 and isinstance(a[8], float) and a[9] is None       # a shared fov: by value, no per-sample array
    assert a[10] == 77.3 and isinstance(a[10], float) and a[11] is None
    one = PanoramaHandler.crop_panorama(torch.rand(64, 128, 3), 60, 24, "16:9")
    assert one.shape == (3, 24, 42)                                        # w = int(h * ratio)
    assert recorder.of("eml_pano_crop_f32")[-1][2] == 1


def test_crop_per_sample_tensors_and_uint8(recorder):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    pano = (torch.rand(2, 64, 128, 3) * 255).to(torch.uint8)
    PanoramaHandler.crop_panorama(pano, _dev([60.0, 90.0]), 24, "4:3", deg=_dev([10.0, -45.0]))
    (a,) = recorder.of("eml_pano_crop_f32")
    assert a[1] == 1 and a[9] is not None and a[11] is not None            # u8 input, per-sample fov and deg arrays
    with pytest.raises(ValueError):
        PanoramaHandler.crop_panorama(pano, 60, 24, "4:3", deg=_dev([1.0, 2.0, 3.0]))     # not one value per sample
    from emlight_amd import _lib
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.crop_panorama(pano, 60, 24, "4:3", deg=torch.tensor([1.0, 2.0]))  # a host tensor
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.crop_panorama(pano.double(), 60, 24)


def test_refused_before_any_launch(recorder):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    from tests.golden.make_golden_panorama import CROP_CASES, CROP_OUT_OF_BOUNDS
    _, (H, W), _, fov, h, aspect, deg, _ = CROP_OUT_OF_BOUNDS
    pano = torch.rand(H, W, 3)
    with pytest.raises(ValueError, match="out of bounds"):
        PanoramaHandler.crop_panorama(pano, fov, h, aspect, deg=deg)        # the reference's interpolator raises here
    for bad in ("4-3", "4:0", "a:b", "4:3:2", "-4:3"):
        with pytest.raises(ValueError):
            PanoramaHandler.crop_panorama(pano, 60, 24, bad)
    for fov in (0, 180, -5):
        with pytest.raises(ValueError):
            PanoramaHandler.crop_panorama(pano, fov, 24)
    with pytest.raises(ValueError):
        PanoramaHandler.resize_panorama(pano, (100, 32))                    # 128 / 100 is no integer factor
    with pytest.raises(ValueError):
        PanoramaHandler.resize_panorama(pano, 24)
    with pytest.raises(ValueError):
        PanoramaHandler.resize_panorama(pano, [64, 32])                     # the reference takes a tuple or an int
    assert recorder.calls == []
    for _, (H, W), _, fov, h, aspect, deg, _ in CROP_CASES:                 # every golden case is inside the bounds
        PanoramaHandler.crop_panorama(torch.rand(H, W, 3), fov, h, aspect, deg=deg)
    assert recorder.calls == ["eml_pano_crop_f32"] * len(CROP_CASES)


# eml_pano_resize_area_f32(pano, B, H, W, h, w, deg, deg_dev, out, stream)
def test_resize_shapes_and_folded_rotation(recorder):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    x = torch.rand(2, 64, 128, 3)
    assert PanoramaHandler.resize_panorama(x, (32, 16), deg=-45.0).shape == (2, 16, 32, 3)    # (w, h)
    assert PanoramaHandler.resize_panorama(x[0], 32).shape == (32, 64, 3)                       # int h -> (2h, h)
    PanoramaHandler.resize_panorama(x, 8, deg=_dev([3.0, 4.0]))
    a, b, c = recorder.of("eml_pano_resize_area_f32")
    assert a[1:8] == (2, 64, 128, 16, 32, -45.0, None)
    assert b[1:8] == (1, 64, 128, 32, 64, 0.0, None)
    assert c[7] is not None
    rolled = PanoramaHandler.horizontal_rotate_panorama(x, 77.3)
    assert torch.equal(rolled, torch.roll(x, int(77.3 / 360.0 * 128), dims=2)) and "roll" not in "".join(recorder.calls)


# eml_tonemap_f32(img, B, n, use_gamma, gamma, percentile, max_mapping, alpha_in, clip, P, out, n_out, stats, work, stream)
def test_tensor_tonemap_reaches_the_kernels(recorder):
    from emlight_amd.RegressionNetwork.util import TonemapHDR
    tone = TonemapHDR(2.4, 99, 0.9)
    out, alpha = tone(torch.rand(4, 3, 8, 12))
    assert out.shape == (4, 3, 8, 12) and alpha.shape == (4,)
    one, a1 = tone(torch.rand(3, 8, 12), clip=False, gamma=False, alpha=0.25)
    assert one.shape == (3, 8, 12) and a1.shape == ()
    assert recorder.calls == ["eml_tonemap_work_floats", "eml_tonemap_f32"] * 2
    a, b = recorder.of("eml_tonemap_f32")
    assert a[1:7] == (4, 288, 1, 2.4, 99.0, 0.9) and a[7] is None and a[8] == 1
    assert b[1:4] == (1, 288, 0) and b[7] is not None and b[8] == 0          # gamma=False, a supplied alpha, clip=False
    with pytest.raises(ValueError):
        tone(torch.rand(8, 12))


def test_cpu_tensor_is_refused_like_everywhere_else():
    from emlight_amd import _lib
    from emlight_amd.RegressionNetwork.util import PanoramaHandler, TonemapHDR
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.crop_panorama(torch.rand(64, 128, 3), 60, 24)
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.resize_panorama(torch.rand(64, 128, 3), 16)
    with pytest.raises(_lib.EmlightHipError):
        TonemapHDR()(torch.rand(3, 8, 8))


def test_numpy_tonemap_calls_nothing_and_is_unchanged(recorder):
    """numpy input keeps the host path bit for bit: restated here as it stood before the tensor path existed."""
    from emlight_amd.RegressionNetwork.util import TonemapHDR
    from tests.golden.make_golden_panorama import TONE_CASES, TONE_SETTINGS, tone_inputs

    def before(self, numpy_img, clip=True, alpha=None, gamma=True):
        img = np.power(numpy_img, 1 / self.gamma) if gamma else numpy_img
        pos = img > 0
        ref = np.percentile(img[pos], self.percentile) if pos.any() else np.percentile(img, self.percentile)
        if alpha is None:
            alpha = self.max_mapping / (ref + 1e-10)
        out = np.multiply(alpha, img)
        if clip:
            out = np.clip(out, 0, 1)
        return out.astype("float32"), alpha

    z = np.load(os.path.join(ROOT, "tests", "golden", "panorama_prep.npz"))
    for name, kind, si, kw in TONE_CASES:
        tone = TonemapHDR(*TONE_SETTINGS[si])
        got, alpha = tone(tone_inputs(kind), **kw)
        want, walpha = before(tone, tone_inputs(kind), **kw)
        assert got.dtype == np.float32 and np.array_equal(got, want) and alpha == walpha, name
        assert np.array_equal(got, z["tone/%s/out" % name]) and float(alpha) == float(z["tone/%s/alpha" % name]), name
    assert recorder.calls == []


def _cpu_mesh(ln, cls=None):
    """An ``extract_mesh`` whose tables live on the host (its constructor needs the device)."""
    if cls is None:
        from emlight_amd.RegressionNetwork.representation import extract_mesh as cls
    m = cls.__new__(cls)
    m.h, m.w, m.ln = 128, 256, ln
    m.csr_pix = torch.arange(128 * 256, dtype=torch.int32)
    m.csr_ptr = torch.zeros(ln + 1, dtype=torch.int32)
    m.lum = torch.tensor([0.3, 0.59, 0.11], dtype=torch.float64)
    return m


def test_batcher_call_sequence_and_output_dict(recorder):
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    bt = PanoramaBatcher(anchors=16, crop_hw=(24, 32), fov_deg=60.0, device="cpu", mesh=_cpu_mesh(16))
    assert bt.aspect == "4:3"
    out = bt(torch.rand(2, 256, 512, 3), deg=_dev([77.3, -45.0]))
    assert recorder.calls == ["eml_pano_crop_f32", "eml_tonemap_work_floats", "eml_tonemap_f32", "eml_pano_resize_area_f32",
                              "eml_gt_parametrise_f64"]                       # extract_mesh after the resize
    crop, resize, gt = (recorder.of(n)[0] for n in ("eml_pano_crop_f32", "eml_pano_resize_area_f32", "eml_gt_parametrise_f64"))
    assert crop[8] == 60.0 and crop[9] is None and crop[11] is not None      # shared fov by value, per-sample deg
    assert resize[1:6] == (2, 256, 512, 128, 256) and resize[7] is not None  # the same rotation, folded into the resize
    assert gt[3:7] == (2, 128, 256, 16)
    tm = recorder.of("eml_tonemap_f32")[0]
    assert tm[1:7] == (2, 3 * 24 * 32, 1, 2.4, 50.0, 0.5)                    # data.py:43
    assert {k: tuple(v.shape) for k, v in out.items()} == {
        "crop": (2, 3, 24, 32), "distribution": (2, 16), "intensity": (2, 1), "rgb_ratio": (2, 3), "ambient": (2, 3),
        "alpha": (2,)}
    assert all(v.dtype == torch.float32 for v in out.values())
    bt(torch.rand(2, 256, 512, 3), deg=10.0, fov_deg=90.0)                     # Python numbers go by value
    crop = recorder.of("eml_pano_crop_f32")[-1]
    assert crop[8] == 90.0 and crop[10] == 10.0 and crop[9] is None and crop[11] is None
    with pytest.raises(ValueError):
        bt(torch.rand(256, 512, 3), deg=0.0)                                   # a batch, not one image


def test_train_pano_dir_parses_and_builds_the_batcher(recorder, monkeypatch, tmp_path):
    from emlight_amd.RegressionNetwork import data, representation, train
    args = train.build_parser().parse_args(["--pano_dir", str(tmp_path), "--fov", "75", "--anchors", "32", "--crop_hw", "24", "32"])
    assert args.pano_dir == str(tmp_path) and args.fov == 75.0
    real = representation.extract_mesh
    monkeypatch.setattr(representation, "extract_mesh", lambda h, w, ln, device: _cpu_mesh(ln, real))
    bt = train.make_batcher(args, "cpu")
    assert isinstance(bt, data.PanoramaBatcher) and (bt.fov_deg, bt.crop_h, bt.crop_w, bt.anchors) == (75.0, 24, 32, 32)
    default = train.build_parser().parse_args(["--synthetic"])
    assert default.pano_dir is None and train.make_batcher(default, "cpu") is None   # the default path is untouched
    with pytest.raises(FileNotFoundError):
        data.PanoramaDataset(str(tmp_path))
    np.save(str(tmp_path / "a.npy"), np.random.default_rng(0).random((8, 16, 3)))
    np.save(str(tmp_path / "b.npy"), np.zeros((8, 16)))
    ds = data.PanoramaDataset(str(tmp_path))
    assert len(ds) == 2 and ds[0]["name"] == "a" and ds[0]["pano"].shape == (8, 16, 3) and ds[0]["pano"].dtype == torch.float32
    with pytest.raises(ValueError):
        ds[1]


def test_header_binding_and_readme_agree():
    from emlight_amd import _lib
    header = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    version = int(re.search(r"#define EML_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == version
    for name, nargs in (("eml_pano_crop_f32", 14), ("eml_pano_resize_area_f32", 10), ("eml_tonemap_f32", 15),
                        ("eml_tonemap_work_floats", 1)):
        decl = re.search(r"\b%s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ABI %d, %d symbols" % (version, len(_lib.SIGNATURES)) in readme
    assert "pano_prep" in readme


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def crop(pano=one, B=1, H=64, W=128, h=24, w=32, ratio=4 / 3, fov=60.0, fov_dev=None, deg=0.0, out=one):
        return L.eml_pano_crop_f32(pano, 0, B, H, W, h, w, ratio, fov, fov_dev, deg, None, out, None)

    assert crop(pano=None) == -1 and b"null" in L.eml_last_error()
    assert crop(out=None) == -1 and b"null" in L.eml_last_error()
    assert crop(B=65536) == -1 and b"grid.y" in L.eml_last_error()
    assert crop(H=1) == -1 and b"bad size" in L.eml_last_error()
    assert crop(w=0) == -1 and b"bad size" in L.eml_last_error()
    assert crop(ratio=0.0) == -1 and b"aspect" in L.eml_last_error()
    assert crop(fov=180.0) == -1 and b"(0, 180)" in L.eml_last_error()
    assert crop(deg=float("nan")) == -1 and b"finite" in L.eml_last_error()
    assert crop(B=0) == 0                                                   # empty batch: nothing to launch

    def resize(pano=one, B=1, H=64, W=128, h=16, w=32, deg=0.0, out=one):
        return L.eml_pano_resize_area_f32(pano, B, H, W, h, w, deg, None, out, None)

    assert resize(pano=None) == -1 and b"null" in L.eml_last_error()
    assert resize(h=24) == -1 and b"integer factors" in L.eml_last_error()
    assert resize(w=100) == -1 and b"integer factors" in L.eml_last_error()
    assert resize(deg=float("inf")) == -1 and b"finite" in L.eml_last_error()
    assert resize(B=0) == 0

    def tone(img=one, B=1, n=96, use_gamma=1, gamma=2.4, q=50.0, P=one, stats=one, work=one):
        return L.eml_tonemap_f32(img, B, n, use_gamma, gamma, q, 0.5, None, 1, P, one, one, stats, work, None)

    assert tone(img=None) == -1 and b"null" in L.eml_last_error()
    assert tone(P=None) == -1 and tone(stats=None) == -1 and tone(work=None) == -1
    assert tone(n=0) == -1 and b"values per image" in L.eml_last_error()
    assert tone(q=100.5) == -1 and tone(q=-1.0) == -1 and b"percentile" in L.eml_last_error()
    assert tone(gamma=0.0) == -1 and b"gamma" in L.eml_last_error()
    assert tone(gamma=0.0, use_gamma=0, B=0) == 0
    assert tone(B=0) == 0
    # scratch: three histograms (2048 + 2048 + 512 counts) and 16 words of selection state per image
    assert L.eml_tonemap_work_floats(3) == 3 * (2048 + 2048 + 512 + 16)
    assert L.eml_tonemap_work_floats(0) == 0
