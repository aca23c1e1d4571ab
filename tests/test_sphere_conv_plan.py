"""CPU: which kernels every SphereConv layer takes (``spherenet._conv_plan``) against a literal table.

The speed records under ``profiles/`` rest on this choice, so it is pinned where no GPU is needed: the plan is pure host
arithmetic over the shape, the need-gradient flags and the two host-only ``*_supported`` queries of the library."""
import pytest

P = ("fwd", "dgrad", "wgrad", "keep", "split")
ALL = (True, True, True)                                     # x, weight and bias need a gradient
LIB_KEPT = ("library", "library", "library", True, 0)        # im2col + library GEMMs, the operand kept for the weight gradient
SMALL, NARROW = ("small",) * 3 + (False, 0), ("narrow",) * 3 + (False, 0)

# Recorded at commit 79314c8 (the parent of the change that introduced ``_conv_plan``) on the MI355X: the entry points each layer
# called in a forward + backward with every gradient wanted, as ``test_sphere_conv_ngf64_layer_shapes_natural_dispatch`` prints
# them (``dispatch ...``), plus the split argument of ``eml_sphere_conv_wgrad_fused_f32``.  keep = the forward's im2col operand
# served the weight gradient (``eml_sphere_im2col_f32`` ran once, not twice).  (B, Cin, Cout, H, W, stride) -> plan
NGF64_PLANS = {
    (32, 3, 128, 4, 8, 1): SMALL, (32, 128, 2048, 4, 8, 1): LIB_KEPT, (32, 1024, 1024, 4, 8, 1): LIB_KEPT,
    (32, 3, 128, 8, 16, 1): SMALL, (32, 128, 2048, 8, 16, 1): LIB_KEPT, (32, 1024, 1024, 8, 16, 1): LIB_KEPT,
    (32, 3, 128, 16, 32, 1): SMALL, (32, 128, 2048, 16, 32, 1): LIB_KEPT, (32, 128, 1024, 16, 32, 1): LIB_KEPT,
    (32, 1024, 512, 16, 32, 1): LIB_KEPT, (32, 512, 512, 16, 32, 1): LIB_KEPT,
    (32, 3, 128, 32, 64, 1): SMALL, (32, 128, 1024, 32, 64, 1): LIB_KEPT, (32, 128, 512, 32, 64, 1): LIB_KEPT,
    (32, 512, 256, 32, 64, 1): ("fused", "library", "fused", False, 14),
    (32, 256, 256, 32, 64, 1): ("fused", "library", "fused", False, 28),
    (32, 3, 128, 64, 128, 1): SMALL, (32, 128, 512, 64, 128, 1): LIB_KEPT,
    (32, 128, 256, 64, 128, 1): ("fused", "fused", "fused", False, 56),
    (32, 256, 128, 64, 128, 1): ("fused", "fused", "fused", False, 56),
    (32, 128, 128, 64, 128, 1): ("fused", "fused", "fused", False, 113),
    (32, 3, 128, 128, 256, 1): SMALL,
    (32, 128, 256, 128, 256, 1): ("fused", "fused", "fused", False, 56),
    (32, 128, 128, 128, 256, 1): ("fused", "fused", "fused", False, 113),
    (32, 128, 64, 128, 256, 1): ("fused", "fused", "fused", False, 113),
    (32, 64, 64, 128, 256, 1): ("fused", "fused", "fused", False, 113),
    (32, 64, 3, 128, 256, 1): NARROW,
    (64, 6, 64, 128, 256, 2): LIB_KEPT,
    (64, 64, 128, 64, 128, 2): ("fused", "library", "fused", False, 113),
    (64, 128, 256, 32, 64, 2): ("fused", "library", "library", False, 0),
    (64, 256, 512, 16, 32, 1): LIB_KEPT, (64, 512, 3, 16, 32, 1): NARROW,
    (64, 6, 64, 64, 128, 2): LIB_KEPT,
    (64, 64, 128, 32, 64, 2): ("fused", "library", "library", False, 0),
    (64, 128, 256, 16, 32, 2): LIB_KEPT, (64, 256, 512, 8, 16, 1): LIB_KEPT, (64, 512, 3, 8, 16, 1): NARROW,
}

# The VGG19 stack of the perceptual loss (planar 3x3 convolutions, ReLU in the epilogue) as one joint step at the benchmark's size
# runs it, recorded the same way at the same commit: with every gradient wanted, and as the step runs the fake branch (frozen
# weights: the input gradient alone).  (B, Cin, Cout, H, W, (need x, weight, bias)) -> plan
X_ONLY = (True, False, False)
VGG_PLANS = {
    (32, 3, 64, 128, 256, ALL): SMALL, (32, 3, 64, 128, 256, X_ONLY): ("small", "small", None, False, 0),
    (32, 64, 64, 128, 256, ALL): ("fused", "fused", "fused", False, 113),
    (32, 64, 64, 128, 256, X_ONLY): ("fused", "fused", None, False, 0),
    (32, 64, 128, 64, 128, ALL): ("fused", "fused", "fused", False, 113),
    (32, 64, 128, 64, 128, X_ONLY): ("fused", "fused", None, False, 0),
    (32, 128, 128, 64, 128, ALL): ("fused", "fused", "fused", False, 113),
    (32, 128, 128, 64, 128, X_ONLY): ("fused", "fused", None, False, 0),
    (32, 128, 256, 32, 64, ALL): ("fused", "library", "fused", False, 56),
    (32, 128, 256, 32, 64, X_ONLY): ("fused", "library", None, False, 0),
    (32, 256, 256, 32, 64, ALL): ("fused", "library", "fused", False, 28),
    (32, 256, 256, 32, 64, X_ONLY): ("fused", "library", None, False, 0),
    (32, 256, 512, 16, 32, ALL): LIB_KEPT, (32, 256, 512, 16, 32, X_ONLY): ("library", "library", None, False, 0),
    (32, 512, 512, 16, 32, ALL): LIB_KEPT, (32, 512, 512, 16, 32, X_ONLY): ("library", "library", None, False, 0),
    (32, 512, 512, 8, 16, ALL): LIB_KEPT, (32, 512, 512, 8, 16, X_ONLY): ("library", "library", None, False, 0),
}

# The edges of each rule at the smallest sizes that cross them, each expectation worked out from the expressions of commit 79314c8
# (``_SphereConvFn.forward``, ``_backward_dispatch``) with fused_min_bytes = 64 MiB; the operand is B * H'W' * 9C * 4 bytes.
# (kind, stride, B, C, O, H, W, residual, slope, (need x, weight, bias)) -> plan
EDGES = [
    # an empty batch launches nothing: ATen's empty GEMMs, the (empty) operand kept
    (("sphere", 1, 0, 64, 64, 128, 256, False, 1.0, ALL), LIB_KEPT),
    # C % 32 != 0: no fused forward (113 MB of operand, O <= 256); C = 32 tiles for the forward but not for either gradient
    (("sphere", 1, 2, 48, 64, 128, 256, False, 1.0, ALL), LIB_KEPT),
    (("sphere", 1, 2, 32, 64, 128, 256, False, 1.0, ALL), ("fused", "library", "library", False, 0)),
    # O % 64 != 0: no fused forward (151 MB of operand); O = 64 has one (65536 pixels < 131072, operand < 256 MiB: library gradients)
    (("sphere", 1, 2, 64, 96, 128, 256, False, 1.0, ALL), LIB_KEPT),
    (("sphere", 1, 2, 64, 64, 128, 256, False, 1.0, ALL), ("fused", "library", "library", False, 0)),
    # the operand on either side of fused_min_bytes (O <= 256): 29056 * 2304 = 66 945 024 < 2^26 <= 67 239 936 = 29184 * 2304
    (("sphere", 1, 1, 64, 64, 128, 227, False, 1.0, ALL), LIB_KEPT),
    (("sphere", 1, 1, 64, 64, 128, 228, False, 1.0, ALL), ("fused", "library", "library", False, 0)),
    # ... and of 32 x that, which a wide layer (O > 256) needs: 14 * 32768 * 4608 < 2^31 <= 15 * 32768 * 4608; the fused weight
    # gradient's split: 9 * 1 * 4 = 36 tiles, min(15360 chunks, 1024 // 36, 512 MiB // 2.25 MiB) = 28
    (("sphere", 1, 14, 128, 512, 128, 256, False, 1.0, ALL), LIB_KEPT),
    (("sphere", 1, 15, 128, 512, 128, 256, False, 1.0, ALL), ("fused", "library", "fused", False, 28)),
    # B * H'W' on either side of 32768 (fused weight gradient; the operand, 288 MiB, is past its 4 x 64 MiB): 18 tiles, 1024 // 18
    (("sphere", 1, 1, 256, 128, 128, 255, False, 1.0, ALL), ("fused", "library", "library", False, 0)),
    (("sphere", 1, 1, 256, 128, 128, 256, False, 1.0, ALL), ("fused", "library", "fused", False, 56)),
    # ... and of 131072 (fused input gradient): 9 tiles, 1024 // 9
    (("sphere", 1, 4, 64, 64, 128, 255, False, 1.0, ALL), ("fused", "library", "fused", False, 113)),
    (("sphere", 1, 4, 64, 64, 128, 256, False, 1.0, ALL), ("fused", "fused", "fused", False, 113)),
    # stride 2 (the same 131072 output pixels): no transposed-table input gradient
    (("sphere", 2, 4, 64, 64, 256, 512, False, 1.0, ALL), ("fused", "library", "fused", False, 113)),
    # a residual excludes the 3-channel-input and the few-output-channel kernels; an activation only the latter (the small
    # kernels fold it in: VGG's conv1_1); so does the planar table
    (("sphere", 1, 2, 3, 128, 8, 16, False, 1.0, ALL), SMALL),
    (("sphere", 1, 2, 3, 128, 8, 16, True, 1.0, ALL), LIB_KEPT),
    (("sphere", 1, 2, 3, 128, 8, 16, False, 0.2, ALL), SMALL),
    (("sphere", 1, 2, 64, 3, 8, 16, False, 1.0, ALL), NARROW),
    (("sphere", 1, 2, 64, 3, 8, 16, True, 1.0, ALL), LIB_KEPT),
    (("sphere", 1, 2, 64, 3, 8, 16, False, 0.2, ALL), LIB_KEPT),
    (("planar", 1, 2, 64, 3, 8, 16, False, 1.0, ALL), LIB_KEPT),
    # a weight without a gradient: no weight-gradient kernel, no kept operand; likewise an input without one
    (("sphere", 1, 32, 128, 2048, 4, 8, False, 1.0, (True, False, True)), ("library", "library", None, False, 0)),
    (("sphere", 1, 32, 128, 2048, 4, 8, False, 1.0, (False, True, True)), ("library", None, "library", True, 0)),
    (("sphere", 1, 32, 128, 128, 128, 256, False, 1.0, (True, False, False)), ("fused", "fused", None, False, 0)),
    (("sphere", 1, 2, 3, 128, 8, 16, False, 1.0, (False, True, True)), ("small", None, "small", False, 0)),
]


def _plan(kind, stride, B, C, O, H, W, res, slope, needs):
    from emlight_amd import _lib
    from emlight_amd.GenProjector import spherenet
    L = _lib.lib()
    return tuple(spherenet._conv_plan(kind, stride, B, C, O, H, W, res, slope, spherenet._Needs(*needs, res),
                                      bool(L.eml_sphere_conv_small_supported(C, O)), bool(L.eml_sphere_conv_narrow_supported(C, O))))


@pytest.fixture(autouse=True)
def _default_tuning(monkeypatch):
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    monkeypatch.setattr(SphereConv2D, "fused_min_bytes", 64 << 20)
    monkeypatch.setattr(SphereConv2D, "wgrad_workgroups", 1024)


def test_ngf64_and_vgg19_layers_take_the_recorded_kernels():
    from tests.test_gpu_projector import NGF64_SHAPES
    assert set(NGF64_PLANS) == set(NGF64_SHAPES)
    got = {s: _plan("sphere", s[5], *s[:5], False, 1.0, ALL) for s in NGF64_PLANS}
    assert got == NGF64_PLANS, {s: (got[s], NGF64_PLANS[s]) for s in got if got[s] != NGF64_PLANS[s]}
    assert len(VGG_PLANS) == 18
    got = {k: _plan("planar", 1, *k[:5], False, 0.0, k[5]) for k in VGG_PLANS}
    assert got == VGG_PLANS, {k: (got[k], VGG_PLANS[k]) for k in got if got[k] != VGG_PLANS[k]}


@pytest.mark.parametrize("args,want", EDGES)
def test_plan_at_the_edges_of_each_rule(args, want):
    assert _plan(*args) == want, dict(zip(P, _plan(*args)))


def test_the_one_launch_spade_asks_for_its_backward_only():
    """``_SpadeConvModulateFn`` runs the forward itself (no im2col operand exists): the plan of its 2 Cn-wide convolution keeps the
    gradient rules of a plain layer, without the kept-operand weight gradient -- 128 -> 512 at 64 x 128, a library forward on its
    own (operand 1.2 GB < 2 GiB, O > 256), takes the fused weight gradient under SPADE (commit 79314c8: ``_backward_dispatch``)."""
    from emlight_amd.GenProjector import spherenet
    needs = spherenet._Needs(True, True, True, False)
    assert _plan("sphere", 1, 32, 128, 512, 64, 128, False, 1.0, ALL) == LIB_KEPT
    got = spherenet._conv_plan("sphere", 1, 32, 128, 512, 64, 128, False, 1.0, needs, False, False, fwd="fused")
    assert tuple(got) == ("fused", "library", "fused", False, 28)
