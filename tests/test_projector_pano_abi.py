"""CPU: the projector's panorama path (csrc/projector_prep.hip: light targets, bilinear resize; ``ProjectorPanoramaBatcher``)
reaches its C ABI entry points with arguments that convert to the bound signatures -- WITHOUT a GPU.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_panorama_prep_abi.py``, restated here).  The
launchers' own argument validation is checked against the built library (it returns before anything touches a device)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"eml_projector_targets_work_floats": 3, "eml_projector_targets_f32": 9, "eml_resize_bilinear_f32": 11}


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
    @property
    def is_cuda(self):
        return True


def _cpu_mesh(ln):
    """An ``extract_mesh`` whose tables live on the host (its constructor needs the device)."""
    from emlight_amd.RegressionNetwork.representation import extract_mesh as cls
    m = cls.__new__(cls)
    m.h, m.w, m.ln = 128, 256, ln
    m.csr_pix = torch.arange(128 * 256, dtype=torch.int32)
    m.csr_ptr = torch.zeros(ln + 1, dtype=torch.int32)
    m.lum = torch.tensor([0.3, 0.59, 0.11], dtype=torch.float64)
    return m


def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    header = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                 # the comments name the entry points too
    for name, nargs in NEW.items():
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(handle, name), "libemlight_hip.so does not export %s" % name
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().eml_abi_version()
    assert "projector_prep" in open(os.path.join(ROOT, "README.md")).read()


def test_a_library_without_the_new_symbols_is_refused(built_lib, monkeypatch):
    """Bound by name: a library from before this header fails at load, not at the first call."""
    from emlight_amd import _lib

    class Old:
        def __getattr__(self, name):
            if name in NEW:
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EmlightHipError, match="lacks symbol eml_(projector_targets|resize_bilinear)"):
        _lib.lib()


# eml_projector_targets_f32(small, alpha, B, h, w, warped, map, work, stream)
def test_light_targets_call(recorder):
    from emlight_amd.GenProjector.data import light_targets
    warped, mask = light_targets(torch.rand(3, 6, 10, 3))
    assert warped.shape == (3, 3, 6, 10) and mask.shape == (3, 1, 6, 10) and warped.dtype == mask.dtype == torch.float32
    assert recorder.calls == ["eml_projector_targets_work_floats", "eml_projector_targets_f32"]
    assert recorder.of("eml_projector_targets_work_floats")[0] == (3, 6, 10)
    a = recorder.of("eml_projector_targets_f32")[0]
    assert a[1] is None and a[2:5] == (3, 6, 10)                       # alpha=None: a null pointer, the kernel multiplies by 1
    light_targets(torch.rand(2, 4, 4, 3), torch.rand(2))
    assert recorder.of("eml_projector_targets_f32")[1][1] is not None
    for bad in (torch.rand(6, 10, 3), torch.rand(2, 6, 10, 4), torch.rand(2, 0, 10, 3)):
        with pytest.raises(ValueError):
            light_targets(bad)
    with pytest.raises(ValueError):
        light_targets(torch.rand(2, 4, 4, 3), torch.rand(3))           # not one alpha per sample


# eml_resize_bilinear_f32(src, alpha, clip, B, C, h, w, oh, ow, out, stream)
def test_resize_bilinear_call(recorder):
    from emlight_amd.GenProjector.data import resize_bilinear
    out = resize_bilinear(torch.rand(2, 3, 24, 32), (128, 96))
    assert out.shape == (2, 3, 128, 96) and out.dtype == torch.float32
    a = recorder.of("eml_resize_bilinear_f32")[0]
    assert a[1] is None and a[2:9] == (0, 2, 3, 24, 32, 128, 96)
    resize_bilinear(torch.rand(2, 3, 7, 5), (4, 9), alpha=torch.rand(2), clip=True)
    b = recorder.of("eml_resize_bilinear_f32")[1]
    assert b[1] is not None and b[2:9] == (1, 2, 3, 7, 5, 4, 9)
    with pytest.raises(ValueError):
        resize_bilinear(torch.rand(3, 7, 5), (4, 9))
    with pytest.raises(ValueError):
        resize_bilinear(torch.rand(1, 3, 7, 5), (0, 9))
    with pytest.raises(ValueError):
        resize_bilinear(torch.rand(2, 3, 7, 5), (4, 9), alpha=torch.rand(1))


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib
    from emlight_amd.GenProjector.data import light_targets, resize_bilinear
    with pytest.raises(_lib.EmlightHipError):
        light_targets(torch.rand(1, 4, 4, 3))
    with pytest.raises(_lib.EmlightHipError):
        resize_bilinear(torch.rand(1, 3, 4, 4), (2, 2))


def _batcher(monkeypatch, regression):
    """The batcher on host tensors: the recorder stands in for the library, the rasteriser's autograd wrapper for itself."""
    from emlight_amd.GenProjector import data
    monkeypatch.setattr(data, "convert_to_panorama",
                        lambda dirs, sizes, colors, pano_hw=(128, 256): torch.zeros(sizes.shape[0], 3, *pano_hw))
    return data.ProjectorPanoramaBatcher(anchors=16, crop_hw=(24, 32), device="cpu", regression=regression, mesh=_cpu_mesh(16))


def test_batcher_call_sequence_and_keys(recorder, monkeypatch):
    bt = _batcher(monkeypatch, False)
    deg = torch.tensor([77.3, -45.0]).as_subclass(_FakeDeviceTensor)
    out = bt(torch.rand(2, 256, 512, 3), deg=deg)
    assert recorder.calls == ["eml_pano_crop_f32", "eml_tonemap_work_floats", "eml_tonemap_f32", "eml_resize_bilinear_f32",
                              "eml_pano_resize_area_f32", "eml_gt_parametrise_f64", "eml_projector_targets_work_floats",
                              "eml_projector_targets_f32"]
    tm = recorder.of("eml_tonemap_f32")[0]
    assert tm[1:7] == (2, 3 * 24 * 32, 1, 2.4, 50.0, 0.5) and tm[8] == 1 and tm[10] is None   # selection only: no full-size output
    rs = recorder.of("eml_resize_bilinear_f32")[0]
    assert rs[1] is not None and rs[2:9] == (1, 2, 3, 24, 32, 128, 128)                       # P with alpha and clip
    tg = recorder.of("eml_projector_targets_f32")[0]
    assert tg[1] is not None and tg[2:5] == (2, 128, 256)
    assert recorder.of("eml_pano_resize_area_f32")[0][7] is not None                          # the same rotation as the crop
    assert {k: tuple(v.shape) for k, v in out.items()} == {
        "input": (2, 3, 128, 256), "crop": (2, 3, 128, 128), "warped": (2, 3, 128, 256), "map": (2, 1, 128, 256),
        "pano": (2, 128, 256, 3), "alpha": (2,)}
    assert all(v.dtype == torch.float32 for v in out.values())


def test_batcher_with_regression_keys_feeds_the_joint_step(recorder, monkeypatch):
    bt = _batcher(monkeypatch, True)
    out = bt(torch.rand(2, 256, 512, 3), deg=10.0, fov_deg=90.0)
    assert recorder.of("eml_tonemap_f32")[0][10] is not None                                  # the encoder reads the full-size crop
    shapes = {k: tuple(v.shape) for k, v in out.items()}
    assert shapes["crop"] == (2, 3, 24, 32) and shapes["crop128"] == (2, 3, 128, 128)
    assert (shapes["distribution"], shapes["intensity"], shapes["rgb_ratio"], shapes["ambient"]) == ((2, 16), (2, 1), (2, 3), (2, 3))
    assert set(shapes) == {"input", "crop", "crop128", "warped", "map", "pano", "alpha", "distribution", "intensity", "rgb_ratio",
                           "ambient"}
    # JointTrainer.projector_inputs takes crop128 when the batch has it, and resizes the crop as before when not
    from emlight_amd import joint
    monkeypatch.setattr(joint, "predicted_gaussian_map", lambda pred, ln, pano_hw: "map")
    tr = joint.JointTrainer.__new__(joint.JointTrainer)
    tr.ln, tr.pano_hw = 16, (128, 256)
    assert tr.projector_inputs(out, {})["crop"] is out["crop128"]
    old = {k: v for k, v in out.items() if k != "crop128"}
    want = torch.nn.functional.interpolate(out["crop"], size=(128, 128), mode="bilinear", align_corners=False)
    assert torch.equal(tr.projector_inputs(old, {})["crop"], want)


def test_the_regression_batcher_is_unchanged(recorder):
    """``PanoramaBatcher`` shares its steps with the projector's batcher now: same calls, same dict."""
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    bt = PanoramaBatcher(anchors=16, crop_hw=(24, 32), device="cpu", mesh=_cpu_mesh(16))
    out = bt(torch.rand(2, 256, 512, 3), deg=12.0)
    assert recorder.calls == ["eml_pano_crop_f32", "eml_tonemap_work_floats", "eml_tonemap_f32", "eml_pano_resize_area_f32",
                              "eml_gt_parametrise_f64"]
    assert list(out) == ["crop", "distribution", "intensity", "rgb_ratio", "ambient", "alpha"]


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def targets(small=one, B=1, h=4, w=4, warped=one, mp=one, work=one):
        return L.eml_projector_targets_f32(small, None, B, h, w, warped, mp, work, None)

    for kw in ({"small": None}, {"warped": None}, {"mp": None}, {"work": None}):
        assert targets(**kw) == -1 and b"null" in L.eml_last_error(), kw
    assert targets(B=-1) == -1 and targets(B=65536) == -1 and b"grid.y" in L.eml_last_error()
    assert targets(h=0) == -1 and b"bad size" in L.eml_last_error()
    assert targets(w=0) == -1 and targets(h=1 << 15, w=1 << 15) == -1 and b"bad size" in L.eml_last_error()
    assert targets(B=0) == 0                                                # empty batch: nothing to launch
    # one partial maximum per (image, slice): a slice per 1024-pixel tile, at most 64 per image
    assert L.eml_projector_targets_work_floats(3, 6, 10) == 3
    assert L.eml_projector_targets_work_floats(2, 33, 33) == 2 * 2
    assert L.eml_projector_targets_work_floats(2, 128, 256) == 2 * 32
    assert L.eml_projector_targets_work_floats(5, 1024, 2048) == 5 * 64
    assert L.eml_projector_targets_work_floats(0, 4, 4) == 0 and L.eml_projector_targets_work_floats(2, 0, 4) == 0

    def resize(src=one, B=1, C=3, h=4, w=4, oh=8, ow=8, out=one):
        return L.eml_resize_bilinear_f32(src, None, 0, B, C, h, w, oh, ow, out, None)

    assert resize(src=None) == -1 and b"null" in L.eml_last_error()
    assert resize(out=None) == -1 and b"null" in L.eml_last_error()
    assert resize(B=-1) == -1 and resize(C=0) == -1 and resize(B=30000, C=3) == -1 and b"grid.y" in L.eml_last_error()
    for kw in ({"h": 0}, {"w": 0}, {"oh": 0}, {"ow": 0}, {"oh": 1 << 15, "ow": 1 << 15}):
        assert resize(**kw) == -1 and b"bad size" in L.eml_last_error(), kw
    assert resize(B=0) == 0
