"""CPU: convert_to_panorama's backward wrt dirs / sizes / colors reaches the C ABI with arguments that convert to the bound
signature, and the colours-only backward keeps its own entry point -- WITHOUT a GPU.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_dry_run_abi.py``, restated here).  The launcher's own
argument validation is checked against the built library (it returns before anything touches a device)."""
import ctypes

import pytest
import torch


class _Recorder:
    def __init__(self, signatures):
        self.signatures, self.calls, self.args = signatures, [], []

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        _, argtypes = self.signatures[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, call site passes %d" % (name, len(argtypes), len(args))
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError("%s: argument %d (%r) does not convert to %s" % (name, k, a, t.__name__)) from e
            self.calls.append(name)
            self.args.append((name, args))
            return 0
        return call


@pytest.fixture
def recorder(monkeypatch):
    from emlight_amd import _lib
    rec = _Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name, dtype=None: t.contiguous())
    return rec


def _inputs(B=2, n=16, grads=(True, True, True)):
    return [torch.rand(B, k * n).requires_grad_(r) for k, r in zip((3, 1, 3), grads)]


@pytest.mark.parametrize("grads", [(True, True, True), (True, False, False), (False, True, False), (True, True, False)])
def test_backward_wrt_dirs_or_sizes_calls_the_full_gradient_entry(recorder, grads):
    from emlight_amd.RegressionNetwork.util import convert_to_panorama
    d, s, c = _inputs(grads=grads)
    convert_to_panorama(d, s, c, pano_hw=(8, 16)).sum().backward()
    assert "eml_sg_rasterise_bwd_colors_ex_f32" not in recorder.calls
    (args,) = [a for n, a in recorder.args if n == "eml_sg_rasterise_bwd_f32"]
    gd, gs, gc = args[4:7]
    assert [p is not None for p in (gd, gs, gc)] == list(grads)       # outputs nobody asked for are NULL
    assert args[8:13] == (2, 16, 8, 16, 0)                            # B, N, H, W, flags (culled)
    assert recorder.calls.index("eml_sg_rasterise_bwd_full_work_floats") < recorder.calls.index("eml_sg_rasterise_bwd_f32")
    for t, want in zip((d, s, c), grads):
        assert (t.grad is not None) == want


def test_colours_only_backward_keeps_the_colour_entry(recorder):
    from emlight_amd.RegressionNetwork.util import convert_to_panorama
    d, s, c = _inputs(grads=(False, False, True))
    convert_to_panorama(d, s, c, pano_hw=(8, 16)).sum().backward()
    assert "eml_sg_rasterise_bwd_colors_ex_f32" in recorder.calls
    assert "eml_sg_rasterise_bwd_f32" not in recorder.calls
    assert c.grad is not None and d.grad is None and s.grad is None


def test_raw_full_gradient_flags_and_partial_requests(recorder):
    from emlight_amd.RegressionNetwork.util import rasterise_bwd_raw
    d, s, c = (t.detach() for t in _inputs())
    gout = torch.rand(2, 3, 8, 16)
    gd, gs, gc = rasterise_bwd_raw(d, s, c, gout, (8, 16), exhaustive=True, need=(False, True, False))
    assert gd is None and gc is None and gs.shape == (2, 16)
    assert recorder.args[-1][1][12] == 1                              # EML_SG_EXHAUSTIVE
    with pytest.raises(ValueError):
        rasterise_bwd_raw(d, s, c, gout, (8, 16), need=(False, False, False))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_full_gradient_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def call(gd=one, gs=one, gc=one, B=1, N=4, H=8, W=16, flags=0, colors=one):
        return L.eml_sg_rasterise_bwd_f32(one, one, colors, one, gd, gs, gc, one, B, N, H, W, flags, None)

    assert call(gd=None, gs=None, gc=None) == -1 and b"null" in L.eml_last_error()
    assert call(colors=None) == -1 and b"null" in L.eml_last_error()
    assert call(W=20) == -1 and b"W==2H" in L.eml_last_error()
    assert call(flags=2) == -1 and b"unknown flags" in L.eml_last_error()
    assert call(B=65536) == -1 and b"grid.z" in L.eml_last_error()
    assert call(B=65535, N=5000) == -1 and b"too many lights" in L.eml_last_error()   # B*N*7 > 2^31 - 1
    assert call(B=0) == 0                                                             # empty batch: nothing to launch
    # per-tile partials: 7 sums per light and tile, tiles of 32 x 16 pixels (partial tiles count whole)
    assert L.eml_sg_rasterise_bwd_full_work_floats(3, 5, 72, 144) == 3 * 5 * 5 * 5 * 7
    assert L.eml_sg_rasterise_bwd_full_work_floats(0, 5, 72, 144) == 0
