"""CPU: ``eml_sphere_conv_small_dbias_f32`` -- the bias gradient of a 3-channel input SphereConv layer without its weight gradient.

* declared in ``include/emlight_hip_ext.h`` (citing the reference's lines), bound in ``_lib.EXT_SIGNATURES`` with a matching
  argument count and exported; the first header keeps its 131 names and ABI 31;
* the launcher validates before it enqueues: bad arguments return EML_EINVAL and a message without a GPU;
* ``_sphere_conv_backward`` calls it exactly where the small family's bias wants a gradient and its weight does not.

Its values -- the bits of the weight-gradient kernel's bias column -- are held on the GPU by tests/test_gpu_sphere_conv_requests.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "eml_sphere_conv_small_dbias_f32"


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
    assert sorted(set(re.findall(r"\b(eml_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.EXT_SIGNATURES)
    decl = re.search(r"\b%s\((.*?)\);" % NAME, code, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[NAME][1]) == 10
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libemlight_hip.so does not export %s" % NAME
    assert getattr(built_lib, NAME).argtypes == _lib.EXT_SIGNATURES[NAME][1] and _lib.EXT_SIGNATURES[NAME][0] is ctypes.c_int
    assert NAME not in first and NAME not in _lib.SIGNATURES
    # the declaration cites the reference
    comment = ext[:ext.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "spherenet/sphere_cnn.py:111-124" in comment and "normalization.py:92-96" in comment
    # the first header, its table and the ABI version are untouched
    assert len(_lib.SIGNATURES) == 131 and not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", first).group(1)) == _lib.ABI_VERSION == 31


def test_launcher_argument_validation_without_gpu(built_lib):
    L, f, one = built_lib, ctypes.c_float, ctypes.c_void_p(16)

    def call(dy=one, y=one, slope=0.2, part=one, db=one, B=1, Po=32, C=3, O=64):
        return L.eml_sphere_conv_small_dbias_f32(dy, y, f(slope), part, db, B, Po, C, O, None)
    for key in ("dy", "part", "db"):
        assert call(**{key: None}) == -1 and b"eml_sphere_conv_small_dbias_f32: null" in L.eml_last_error(), key
    for kw in ({"B": -1}, {"Po": 0}):
        assert call(**kw) == -1 and b"empty shape" in L.eml_last_error(), kw
    for kw in ({"C": 6}, {"O": 96}, {"C": 4, "O": 128}):
        assert call(**kw) == -1 and b"(C, O)" in L.eml_last_error(), kw
    for kw in ({"slope": 1.5}, {"slope": -0.1}, {"slope": 0.0, "y": None}, {"slope": 0.2, "y": None}):
        assert call(**kw) == -1 and b"act_slope" in L.eml_last_error(), kw
    assert call(B=1 << 16, Po=1 << 15) == -1 and b"too many pixels" in L.eml_last_error()


def test_backward_calls_it_for_the_bias_without_the_weight_only(built_lib, monkeypatch):
    """``_sphere_conv_backward`` on the CPU with the library replaced by a recorder: the plan of a 3 -> 64 layer, every request."""
    import torch
    from emlight_amd import _lib
    from emlight_amd.GenProjector import spherenet
    calls = []

    class Recorder:
        def __getattr__(self, name):
            if name.endswith("_floats"):
                return lambda *a: 16

            def call(*a):
                assert len(a) == len({**_lib.SIGNATURES, **_lib.EXT_SIGNATURES}[name][1]), name
                calls.append(name)
                return 0
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    B, C, H, W, O = 2, 3, 4, 8, 64
    geo = type("Geo", (), {"ho": H, "wo": W, "idx": torch.zeros(1, dtype=torch.int32), "wgt": torch.zeros(1),
                           "csr_ptr": torch.zeros(1, dtype=torch.int32), "csr_src": torch.zeros(1, dtype=torch.int32),
                           "csr_w": torch.zeros(1)})()
    xr, w, y = torch.zeros(B, H, W, C), torch.zeros(O, C, 3, 3), torch.zeros(B * H * W, O)
    gy = torch.zeros(B, O, H, W)
    for nx in (False, True):
        for nw in (False, True):
            for nb in (False, True):
                needs = spherenet._Needs(nx, nw, nb, False)
                plan = spherenet._conv_plan("sphere", 1, B, C, O, H, W, False, 0.0, needs, True, False)
                assert plan.fwd == "small"
                del calls[:]
                gx, gw, gb, _ = spherenet._sphere_conv_backward(plan, geo, (B, C, H, W, O), needs, gy, (xr, w, y), True, 0.0)
                assert (NAME in calls) == (nb and not nw), (needs, calls)
                assert ("eml_sphere_conv_small_wgrad_f32" in calls) == nw, (needs, calls)
                assert (gb is not None) == nb and (gw is not None) == nw and (gx is not None) == nx, needs
