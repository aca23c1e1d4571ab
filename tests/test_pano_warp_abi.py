"""CPU: the panorama warp (csrc/pano_warp.hip, ``PanoramaHandler.warp_panorama``, ``GenProjector.data.resize_exr``, the
batchers' ``warp=`` / ``move_range=``, ``--warp_move``) WITHOUT a GPU.

* ``tests/warp_oracle.py`` is pinned to the reference: its positions lie within the stored ``d_ref`` of the maps that the
  reference's own ``resize_exr`` made (``tests/golden/warp.npz``), in chord distance on the sphere.
* The entry point is declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` and exported; the first
  header and its 131 names are untouched.
* The launcher's own argument validation runs against the built library (it returns before anything touches a device).
* The Python layers reach the entry point with arguments that convert to the bound signature: the HIP library is replaced
  by a recorder (the pattern of ``test_projector_pano_abi.py``, restated here)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import warp_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "eml_pano_warp_f32", 13
# the stored d_ref came from this same comparison; another libm may differ in the last bit of a float64 sine, which moves a
# chord of order 1e-6 by some 1e-16
D_REF_SLACK = 1e-12


# ------------------------------------------------------------------------------------------------ oracle vs reference
def test_oracle_is_pinned_to_the_reference_maps():
    z = np.load(os.path.join(ROOT, "tests", "golden", "warp.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "warp.npz")) < 200 * 1024
    seen = 0
    for k, (theta, phi, move) in enumerate(oracle.PARAMS):
        for shape in oracle.SHAPES:
            H, W, h, w = shape
            name = oracle.case_name(k, shape)
            row, col, d_ref = z[name + "/row"], z[name + "/col"], float(z[name + "/d_ref"])
            assert row.dtype == col.dtype == np.float32 and row.shape == col.shape == (h, w)
            mine = oracle.positions(H, W, h, w, theta, phi, move)
            d = oracle.chord(row, col, mine[0], mine[1], H, W)
            print("%-22s chord %.3e, stored %.3e" % (name, d, d_ref))
            assert d <= d_ref + D_REF_SLACK, name
            assert d_ref <= 1.51e-5, name          # float32 accuracy: the reference's matrices and grids are float32
            seen += 1
    assert seen == 16 and len(z.files) == 3 * seen


def test_oracle_conventions():
    """No half-pixel offset, identity at (0, 0, 0); a negative move steps toward +z, which the middle column shows: what
    lies there comes closer and looks larger, so the output columns next to the middle one read the source nearer to it."""
    row, col = oracle.positions(16, 32, 16, 32)
    assert np.abs(row - np.arange(16)[:, None]).max() < 1e-12
    assert np.abs((col - np.arange(32)[None, :] + 16) % 32 - 16).max() < 1e-12
    _, near = oracle.positions(16, 32, 16, 32, move=-0.5)
    assert 16.5 < near[8, 17] < 16.8 and 15.2 < near[8, 15] < 15.5 and abs(near[8, 16] - 16) < 1e-9
    # wrap-bilinear: the last row blends with row 0, the last column with column 0, size and size + 0 land on index 0
    img = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)
    got = oracle.sample(img, np.array([1.5, 2.0, 0.0, np.nan]), np.array([0.0, 3.0, 2.25, 0.0]))
    np.testing.assert_array_equal(got[0], (img[1, 0] + img[0, 0]) / 2)
    np.testing.assert_array_equal(got[1], img[0, 0])
    np.testing.assert_array_equal(got[2], (0.75 * img[0, 2].astype(np.float64) + 0.25 * img[0, 0]).astype(np.float32))
    assert np.isnan(got[3]).all()


# ------------------------------------------------------------------------------------------------ where the symbol lives
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_symbol_is_declared_in_the_extension_header_bound_and_exported(built_lib):
    from emlight_amd import _lib
    ext = open(os.path.join(ROOT, "include", "emlight_hip_ext.h")).read()
    first = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    declared = sorted(set(re.findall(r"\b(eml_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_lib.EXT_SIGNATURES) and NAME in declared
    decl = re.search(r"\b%s\((.*?)\);" % NAME, code, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[NAME][1]) == NARGS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libemlight_hip.so does not export %s" % NAME
    assert built_lib.eml_pano_warp_f32.argtypes == _lib.EXT_SIGNATURES[NAME][1]
    # every declaration of the extension header cites the reference
    assert re.search(r"GenProjector/util\.py:279-343", ext)
    # the first header, its table and the ABI version are untouched
    assert NAME not in first and NAME not in _lib.SIGNATURES and not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    assert len(_lib.SIGNATURES) == 131
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", first).group(1)) == _lib.ABI_VERSION == 31
    assert "EML_ABI_VERSION" not in code
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ABI 31, 131 symbols" in readme and "emlight_hip_ext.h" in readme and "pano_warp.hip" in readme


def test_a_library_without_the_symbol_is_refused(built_lib, monkeypatch):
    from emlight_amd import _lib

    class Old:
        def __getattr__(self, name):
            if name == NAME:
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EmlightHipError, match="lacks symbol %s" % NAME):
        _lib.lib()


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def warp(pano=one, B=1, H=4, W=8, h=4, w=8, theta=0.0, phi=0.0, move=0.0, params=None, out=one, coords=None):
        return L.eml_pano_warp_f32(pano, B, H, W, h, w, theta, phi, move, params, out, coords, None)

    for kw in ({"pano": None}, {"out": None}):
        assert warp(**kw) == -1 and b"null" in L.eml_last_error(), kw
    assert warp(B=-1) == -1 and warp(B=65536) == -1 and b"grid.y" in L.eml_last_error()
    for kw in ({"H": 0}, {"W": 0}, {"h": 0}, {"w": -3}, {"H": 1 << 15, "W": (1 << 14) + 1}, {"h": 1 << 15, "w": 1 << 15}):
        assert warp(**kw) == -1 and b"bad size" in L.eml_last_error(), kw
    for kw in ({"theta": math.nan}, {"phi": math.inf}, {"move": -math.inf}, {"move": math.nan}):
        assert warp(**kw) == -1 and b"not finite" in L.eml_last_error(), kw
    assert warp(B=0) == 0                                   # empty batch: nothing to launch
    assert warp(B=0, coords=one) == 0 and warp(B=0, params=one, move=math.nan) == 0   # per-sample: by-value ones are unused


# ------------------------------------------------------------------------------------------------ recorder
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
    rec = _Recorder({**_lib.SIGNATURES, **_lib.EXT_SIGNATURES})
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", require)
    return rec


class _FakeDeviceTensor(torch.Tensor):
    @property
    def is_cuda(self):
        return True


def _dev(values):
    return torch.tensor(values, dtype=torch.float32).as_subclass(_FakeDeviceTensor)


def _cpu_mesh(ln):
    """An ``extract_mesh`` whose tables live on the host (its constructor needs the device)."""
    from emlight_amd.RegressionNetwork.representation import extract_mesh as cls
    m = cls.__new__(cls)
    m.h, m.w, m.ln = 128, 256, ln
    m.csr_pix = torch.arange(128 * 256, dtype=torch.int32)
    m.csr_ptr = torch.zeros(ln + 1, dtype=torch.int32)
    m.lum = torch.tensor([0.3, 0.59, 0.11], dtype=torch.float64)
    return m


# eml_pano_warp_f32(pano, B, H, W, h, w, theta_deg, phi_deg, move, params_dev, out, coords, stream)
def test_warp_panorama_call(recorder):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    out = PanoramaHandler.warp_panorama(torch.rand(3, 8, 16, 3), (10, 6), theta=25.0, phi=-200, move=0.4)
    assert out.shape == (3, 6, 10, 3) and out.dtype == torch.float32
    a = recorder.of(NAME)[0]
    assert a[1:9] == (3, 8, 16, 6, 10, 25.0, -200.0, 0.4) and a[9] is None and a[11] is None and a[12] is None
    # an int is the height of a 2:1 panorama, None keeps the size; a single image comes back single
    assert PanoramaHandler.warp_panorama(torch.rand(8, 16, 3), 5).shape == (5, 10, 3)
    assert recorder.of(NAME)[1][1:6] == (1, 8, 16, 5, 10)
    img, coords = PanoramaHandler.warp_panorama(torch.rand(8, 16, 3), return_coords=True)
    assert img.shape == (8, 16, 3) and coords.shape == (8, 16, 2) and coords.dtype == torch.float64
    assert recorder.of(NAME)[2][1:6] == (1, 8, 16, 8, 16) and recorder.of(NAME)[2][11] is not None
    _, coords = PanoramaHandler.warp_panorama(torch.rand(4, 8, 16, 3), (4, 2), move=0.1, return_coords=True)
    assert coords.shape == (1, 2, 4, 2)                                     # by value: one set for the batch
    n = len(recorder.calls)
    assert PanoramaHandler.warp_panorama(torch.rand(0, 8, 16, 3), (4, 2)).shape == (0, 2, 4, 3) and len(recorder.calls) == n
    # any tensor parameter: the three travel as one (B, 3) float64 array, the by-value arguments are unused
    recorder.args.clear()
    img, coords = PanoramaHandler.warp_panorama(torch.rand(2, 8, 16, 3), None, theta=5.0, move=_dev([0.25, -0.5]),
                                                return_coords=True)
    assert coords.shape == (2, 8, 16, 2)
    b = recorder.of(NAME)[0]
    assert b[6:9] == (0.0, 0.0, 0.0) and b[9] is not None
    packed = _packed_params(recorder, PanoramaHandler, torch.rand(2, 8, 16, 3), theta=5.0, move=_dev([0.25, -0.5]))
    assert packed.dtype == torch.float64 and packed.is_contiguous()
    assert torch.equal(packed, torch.tensor([[5.0, 0.0, 0.25], [5.0, 0.0, -0.5]], dtype=torch.float64))
    packed = _packed_params(recorder, PanoramaHandler, torch.rand(2, 8, 16, 3), theta=_dev(30.0), phi=_dev([1.0, 2.0]))
    assert torch.equal(packed, torch.tensor([[30.0, 1.0, 0.0], [30.0, 2.0, 0.0]], dtype=torch.float64))   # 0-d: for all


def _packed_params(recorder, handler, pano, **kw):
    """The (B, 3) tensor behind the params pointer of the next call (found through ``torch.stack``)."""
    made = []
    real = torch.stack

    def stack(tensors, dim=0):
        made.append(real(tensors, dim=dim))
        return made[-1]
    torch.stack = stack
    try:
        handler.warp_panorama(pano, None, **kw)
    finally:
        torch.stack = real
    assert len(made) == 1 and recorder.of(NAME)[-1][9].value == made[0].data_ptr()
    return made[0]


def test_warp_panorama_refuses_bad_arguments(recorder):
    from emlight_amd import _lib
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    pano = torch.rand(2, 8, 16, 3)
    for kw in ({"theta": math.nan}, {"phi": math.inf}, {"move": -math.inf}):
        with pytest.raises(ValueError, match="finite"):
            PanoramaHandler.warp_panorama(pano, **kw)
    for shape in ((0, 4), (4, 0), (1, 2, 3), "8x16", 0, 2.5):
        with pytest.raises(ValueError):
            PanoramaHandler.warp_panorama(pano, shape)
    for bad in (torch.rand(8, 16), torch.rand(2, 8, 16, 4), torch.rand(2, 2, 8, 16, 3)):
        with pytest.raises(ValueError):
            PanoramaHandler.warp_panorama(bad)
    with pytest.raises(ValueError, match="one value per sample"):
        PanoramaHandler.warp_panorama(pano, move=_dev([0.1, 0.2, 0.3]))
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.warp_panorama(pano, move=torch.tensor([0.1, 0.2]))      # a host tensor
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.warp_panorama(pano.double())
    assert recorder.calls == []


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib
    from emlight_amd.GenProjector.data import resize_exr
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.warp_panorama(torch.rand(1, 4, 8, 3))
    with pytest.raises(_lib.EmlightHipError):
        resize_exr(torch.rand(4, 8, 3), 4, 8)


def test_resize_exr_mirrors_the_reference_signature(recorder):
    """``res_x`` is ROWS (``util.py:282,312``: ``img_x = img.shape[0]``, ``indx = arange(res_x)`` down the rows)."""
    import inspect
    from emlight_amd.GenProjector.data import resize_exr
    sig = inspect.signature(resize_exr)
    assert list(sig.parameters) == ["img", "res_x", "res_y", "theta", "phi", "move"]
    assert [sig.parameters[k].default for k in ("res_x", "res_y", "theta", "phi", "move")] == [512, 512, 0.0, 0.0, 0.0]
    out = resize_exr(torch.rand(8, 16, 3), 6, 10, move=-0.3)
    assert out.shape == (6, 10, 3)
    assert recorder.of(NAME)[0][1:9] == (1, 8, 16, 6, 10, 0.0, 0.0, -0.3)
    assert resize_exr(torch.rand(2, 8, 16, 3)).shape == (2, 512, 512, 3)
    assert recorder.of(NAME)[1][1:6] == (2, 8, 16, 512, 512)


# ------------------------------------------------------------------------------------------------ batchers
TODAY_PROJECTOR = ["eml_pano_crop_f32", "eml_tonemap_work_floats", "eml_tonemap_f32", "eml_resize_bilinear_f32",
                   "eml_pano_resize_area_f32", "eml_gt_parametrise_f64", "eml_projector_targets_work_floats",
                   "eml_projector_targets_f32"]
TODAY_REGRESSION = ["eml_pano_crop_f32", "eml_tonemap_work_floats", "eml_tonemap_f32", "eml_pano_resize_area_f32",
                    "eml_gt_parametrise_f64"]


def _with_warp(calls):
    k = calls.index("eml_pano_resize_area_f32") + 1
    return calls[:k] + [NAME] + calls[k:]


def _projector_batcher(monkeypatch, **kw):
    from emlight_amd.GenProjector import data
    monkeypatch.setattr(data, "convert_to_panorama",
                        lambda dirs, sizes, colors, pano_hw=(128, 256): torch.zeros(sizes.shape[0], 3, *pano_hw))
    return data.ProjectorPanoramaBatcher(anchors=16, crop_hw=(24, 32), device="cpu", mesh=_cpu_mesh(16), **kw)


def _regression_batcher(**kw):
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    return PanoramaBatcher(anchors=16, crop_hw=(24, 32), device="cpu", mesh=_cpu_mesh(16), **kw)


@pytest.mark.parametrize("kind", ["projector", "regression"])
def test_batchers_make_todays_calls_without_a_warp_and_one_more_with(recorder, monkeypatch, kind):
    make = (lambda **kw: _projector_batcher(monkeypatch, **kw)) if kind == "projector" else _regression_batcher
    today = TODAY_PROJECTOR if kind == "projector" else TODAY_REGRESSION
    panos = torch.rand(2, 256, 512, 3)
    plain = make()(panos, deg=12.0)
    assert recorder.calls == today
    recorder.calls.clear(), recorder.args.clear()
    out = make()(panos, deg=12.0, warp=(10.0, -20.0, 0.5))
    assert recorder.calls == _with_warp(today)
    a = recorder.of(NAME)[0]
    assert a[1:9] == (2, 128, 256, 128, 256, 10.0, -20.0, 0.5) and a[9] is None and a[11] is None
    # the warp reads what the resize wrote, and the targets read what the warp wrote; the crop is made before both
    assert a[0].value == recorder.of("eml_pano_resize_area_f32")[0][8].value
    assert recorder.of("eml_gt_parametrise_f64")[0][0].value == a[10].value
    if kind == "projector":
        assert recorder.of("eml_projector_targets_f32")[0][0].value == a[10].value and out["pano"].data_ptr() == a[10].value
    assert list(out) == list(plain) and all(out[k].shape == plain[k].shape for k in out)
    # a (B, 3) device tensor: per-sample parameters
    recorder.calls.clear(), recorder.args.clear()
    make()(panos, deg=12.0, warp=_dev([[0.0, 0.0, 0.1], [5.0, 6.0, -0.2]]))
    assert recorder.calls == _with_warp(today) and recorder.of(NAME)[0][9] is not None
    for bad in ((1.0, 2.0), _dev([[0.0, 0.0, 0.1]]), _dev([0.0, 0.0, 0.1])):
        with pytest.raises(ValueError):
            make()(panos, deg=12.0, warp=bad)


@pytest.mark.parametrize("kind", ["projector", "regression"])
def test_move_range_draws_after_the_azimuth_from_the_batchers_generator(recorder, monkeypatch, kind):
    make = (lambda **kw: _projector_batcher(monkeypatch, **kw)) if kind == "projector" else _regression_batcher
    today = TODAY_PROJECTOR if kind == "projector" else TODAY_REGRESSION
    draws = []

    def rand(self, B):
        draws.append(B)
        return _dev([0.25] * B).double().as_subclass(_FakeDeviceTensor)
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    monkeypatch.setattr(PanoramaBatcher, "_rand", rand)
    panos = torch.rand(2, 256, 512, 3)
    bt = make(move_range=(-0.6, 0.2))
    bt(panos)
    assert draws == [2, 2] and recorder.calls == _with_warp(today)          # the azimuths, then the moves
    assert recorder.of(NAME)[0][9] is not None
    assert torch.equal(bt.random_move(2), torch.full((2,), -0.6 + 0.25 * 0.8, dtype=torch.float64))
    # a warp passed to the call wins over the drawn one; a given azimuth still leaves the move drawn
    draws.clear(), recorder.calls.clear(), recorder.args.clear()
    bt(panos, deg=3.0, warp=(0.0, 0.0, 0.0))
    assert draws == [] and recorder.of(NAME)[0][9] is None
    bt(panos, deg=3.0)
    assert draws == [2]
    # no move_range: nothing but the azimuths is drawn, nothing is warped
    draws.clear(), recorder.calls.clear()
    make()(panos)
    assert draws == [2] and recorder.calls == today
    for bad in ((0.5, 0.1), (0.0, math.nan), (1.0,)):
        with pytest.raises((ValueError, IndexError)):
            make(move_range=bad)


# ------------------------------------------------------------------------------------------------ command lines
def test_warp_move_flag_is_parsed_and_refused_without_pano_dir(capsys):
    from emlight_amd import joint
    from emlight_amd.GenProjector import options
    from emlight_amd.GenProjector import train as gp_train
    from emlight_amd.RegressionNetwork import data
    from emlight_amd.RegressionNetwork import train as reg_train
    for parser in (reg_train.build_parser(), joint.build_parser(), options.train_parser()):
        args = parser.parse_args(["--pano_dir", "panos", "--warp_move", "-0.6", "0"])
        assert args.warp_move == [-0.6, 0.0] and data.warp_move_range(args) == (-0.6, 0.0)
        assert parser.parse_args(["--pano_dir", "panos"]).warp_move is None
        assert data.warp_move_range(parser.parse_args([])) is None
        with pytest.raises(SystemExit, match="--pano_dir"):
            data.warp_move_range(parser.parse_args(["--warp_move", "-0.6", "0"]))
        with pytest.raises(SystemExit, match="LO <= HI"):
            data.warp_move_range(parser.parse_args(["--pano_dir", "panos", "--warp_move", "0.5", "0"]))
        with pytest.raises(SystemExit):
            parser.parse_args(["--pano_dir", "panos", "--warp_move", "0.5"])        # two values
    capsys.readouterr()
    # the mains refuse it before anything else happens
    for main in (reg_train.main, joint.main, gp_train.main):
        with pytest.raises(SystemExit, match="--warp_move applies to the batches made from --pano_dir"):
            main(["--synthetic", "--warp_move", "-0.6", "0"] if main is not joint.main else ["--warp_move", "-0.6", "0"])
    assert gp_train.parse_args(["--pano_dir", "panos", "--warp_move", "-0.5", "0.25"]).move_range == (-0.5, 0.25)
    assert gp_train.parse_args(["--pano_dir", "panos"]).move_range is None
