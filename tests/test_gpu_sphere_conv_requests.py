"""GPU: SphereConv and SPADE under every gradient-request subset, per kernel path.

``_SphereConvFn`` / ``_sphere_conv_backward`` / ``_conv_plan`` (emlight_amd/GenProjector/spherenet.py) branch on the kernel family,
the epilogue, the transposed tap table, the bias and on WHICH gradients autograd asked for (``_Needs``).  Training asks for partial
sets on every step (frozen discriminators and VGG: x alone; a detached first-layer input: weight and bias alone), so here every
kernel path runs once with every present input (x, weight, bias, residual) requiring a gradient and once for every other
non-empty subset of them, from one set of seeded channels-last inputs and one ``gy``:

a. the forward output of every subset run repeats the full run's bits;
b. so does every requested gradient;
c. nothing runs for a gradient nobody asked for, and the full run calls exactly the entry points of its ``_conv_plan``;
d. the full run against the float64 restatement of ``tests/sphere_conv_oracle.py``, ELEMENTWISE: rtol 1e-4, atol 1e-4 of the
   reference's largest entry (the project's bound for the same quantities against float32 stock ops; an exact reference can only
   be easier to meet); with an activation the gradients are the oracle's under the DEVICE output's own mask, and wherever the
   device's sign differs from the float64 output's, |y64| is within the output bound -- which is what makes that mask legitimate;
e. an empty batch: dx of shape (0, Cin, H, W), dW and db exactly zero, no kernel launched.

Then ``spade_norm_modulate`` in one launch and in two, BatchNorm in training and eval mode, under eight request sets.

Measured on the MI355X, worst ratio to the bound of (d) over output and gradients, per configuration (ids as pytest prints them);
no output of any configuration lies on the other side of zero from its float64 value:

    small, all twelve (2x3x64x8x16 and 2x3x128x8x16; slope 1 / 0.2 / 0; bias on / off)    0.002 or less
    narrow-project 2x64x3x16x32 0.002 (without a bias 0.002)   2x192x2x12x24 stride 2 0.002   2x512x3x8x16 0.003   1x64x3x2x4 0.001
    narrow-onepass 2x64x3x16x32 0.001                           narrow-shape-activation 2x64x3x16x32 slope 0.2 0.004
    fused 2x64x64x8x16 0.006 (residual + 0.2: 0.005, without a bias 0.006)   2x32x64x8x16 0.004   3x128x64x16x32 stride 2 0.008
          2x64x128x8x16 0.009   2x64x128x16x32 stride 2 0.006   2x128x64x8x16 0.007   2x128x128x8x16 0.008   1x64x64x8x16 0.006
    library 2x16x8x8x16 0.003   2x6x12x16x32 stride 2 0.002 (residual + ReLU 0.002)
    lowres 2x128x128x8x16 residual + 0.2 0.004   5x128x128x4x8 ReLU 0.004
    planar 2x64x64x8x16 ReLU 0.004   2x3x64x16x32 ReLU 0.001

What the matrix found, first run on the MI355X:

1. One-launch SPADE, requests {wg, wb, bg, bb}, {wg} and {wb, bb} (heads with the guide map detached): ``AttributeError: 'NoneType'
   object has no attribute 'is_leaf'`` -- ``_sphere_conv_backward`` looked at a weight it is only handed for the input gradient.
   Fixed in spherenet.py.
2. Two-launch SPADE, every request without x: ``eml_bn_bwd_apply_f32`` / ``eml_bn_bwd_apply_up2_f32`` ran for a dx nobody asked for.
   Fixed in spherenet.py (``need_dx``, as the one-launch path already had it).
3. (b) failed on the small path for the requests {bias} and {x, bias}, in all seven configurations of that path that have a bias
   (six "small", one "planar" 2x3x64x16x32).  With the weight the bias gradient is a column of the one-pass weight-gradient
   kernel's MFMA product (``eml_sphere_conv_small_wgrad_f32``); without it that kernel must not run (c), and the same sum was taken
   by the activation backward + ``sum(0)`` of the library, in another order: 45 to 108 of the 64 / 128 entries differed, by at most
   9.5e-6 at max |db| = 30 to 63 (one or two units in the last place), both at 0.001 of the bound of (d).  No host-side change
   makes the two equal: ``eml_sphere_conv_small_dbias_f32`` now runs the same MFMA sequence on the bias column alone (on its own
   at 15, 231, 10 725 and 72 864 pixels: the weight-gradient kernel's bits, 0.002 of the bound or less against float64).
"""
import functools
import itertools
from collections import namedtuple

import pytest
import torch

from tests import sphere_conv_oracle as oracle
from tests.test_gpu_projector import _spy_on_lib

pytestmark = pytest.mark.gpu

NAMES = oracle.NAMES
Config = namedtuple("Config", "path kind shape bias residual slope switches")


def _c(path, shape, bias=True, residual=False, slope=1.0, kind="sphere", **switches):
    return Config(path, kind, shape, bias, residual, slope, tuple(sorted(switches.items())))


# One row per kernel path at the smallest shapes that select it: (B, Cin, Cout, H, W, stride).  The switches are the existing ones
# (SphereConv2D.fused_min_bytes = 0: every layer counts as large; lowres = "force"; narrow_project).
CONFIGS = (
    # the 3-channel input layers, activation and bias gradient folded into their one-pass kernels
    [_c("small", (2, 3, O, 8, 16, 1), bias=b, slope=s) for O in (64, 128) for s in (1.0, 0.2, 0.0) for b in (True, False)]
    # few output channels, project-then-gather: conv_img's width; stride 2; C > 128 (one-pass input gradient); a geometry with no
    # transposed table (one-pass weight gradient, dY W2 + col2im)
    + [_c("narrow-project", s, narrow_project=True) for s in ((2, 64, 3, 16, 32, 1), (2, 192, 2, 12, 24, 2), (2, 512, 3, 8, 16, 1),
                                                               (1, 64, 3, 2, 4, 1))]
    + [_c("narrow-project", (2, 64, 3, 16, 32, 1), bias=False, narrow_project=True)]
    + [_c("narrow-onepass", (2, 64, 3, 16, 32, 1), narrow_project=False)]
    # the same shape with an activation leaves the family: library kernels, O <= 8: the bias gradient by eml_colsum_f32
    + [_c("narrow-shape-activation", (2, 64, 3, 16, 32, 1), slope=0.2)]
    # fused gather-GEMMs; C = 32: both gradients fall to the library, the operand rebuilt; stride 2: the input gradient does
    + [_c("fused", (2, 64, 64, 8, 16, 1), fused_min_bytes=0), _c("fused", (2, 64, 64, 8, 16, 1), residual=True, slope=0.2, fused_min_bytes=0),
       _c("fused", (2, 64, 64, 8, 16, 1), bias=False, fused_min_bytes=0),
       _c("fused", (2, 32, 64, 8, 16, 1), fused_min_bytes=0), _c("fused", (3, 128, 64, 16, 32, 2), fused_min_bytes=0)]
    # one row per instantiation of csrc/sphere_conv_fused.hip the rows above leave out.  Forward: the gather-GEMM's 128-channel
    # tile with row-shared corners (stride 1, O = 128) and without (stride 2).  Weight gradient, (BN, BMO) from (C, O): (64, 128),
    # (128, 64), (128, 128) -- (64, 64) is the first row -- at 2 x 128 pixels: 8 K-splits, the tiles of a split on one XCD; and
    # one sample alone: 4 K-splits, natural tile order
    + [_c("fused", s, fused_min_bytes=0) for s in ((2, 64, 128, 8, 16, 1), (2, 64, 128, 16, 32, 2), (2, 128, 64, 8, 16, 1),
                                                   (2, 128, 128, 8, 16, 1), (1, 64, 64, 8, 16, 1))]
    # im2col + library GEMMs with the operand kept, natural dispatch
    + [_c("library", (2, 16, 8, 8, 16, 1)), _c("library", (2, 6, 12, 16, 32, 2)), _c("library", (2, 6, 12, 16, 32, 2), residual=True, slope=0.0)]
    # the footprint gather-GEMM, forward and input gradient
    + [_c("lowres", (2, 128, 128, 8, 16, 1), residual=True, slope=0.2, lowres="force"),
       _c("lowres", (5, 128, 128, 4, 8, 1), slope=0.0, lowres="force")]
    # planar_conv3x3 (VGG's convolutions, ReLU epilogue): the fused kernels on the single-entry table; conv1_1 on the small ones
    + [_c("planar", (2, 64, 64, 8, 16, 1), slope=0.0, kind="planar", fused_min_bytes=0),
       _c("planar", (2, 3, 64, 16, 32, 1), slope=0.0, kind="planar")]
    # an empty batch: ATen's empty GEMMs
    + [_c("empty", (0, 8, 8, 8, 16, 1)), _c("empty", (0, 3, 64, 8, 16, 1)), _c("empty", (0, 64, 3, 8, 16, 1))]
)
NONEMPTY = [c for c in CONFIGS if c.shape[0] > 0]
EMPTY = [c for c in CONFIGS if c.shape[0] == 0]
PATHS = ("small", "narrow-project", "narrow-onepass", "narrow-shape-activation", "fused", "library", "lowres", "planar", "empty")

WGRAD_ONLY = ("eml_sphere_conv_small_wgrad_f32", "eml_sphere_conv_narrow_wgrad_f32", "eml_sphere_conv_narrow_wgrad2_f32",
              "eml_sphere_conv_wgrad_fused_f32")
SMALL_DBIAS = "eml_sphere_conv_small_dbias_f32"
DGRAD_ONLY = ("eml_sphere_conv_small_da9_f32", "eml_sphere_col2im_f32", "eml_sphere_conv_narrow_dgrad_f32",
              "eml_sphere_conv_narrow_dgrad2_f32", "eml_sphere_conv_dgrad_fused_f32")


def _id(cfg):
    return "%s-%s-%s%s%s%s" % (cfg.path, "x".join(map(str, cfg.shape)), "b" if cfg.bias else "nob", "-res" if cfg.residual else "",
                               "-slope%g" % cfg.slope if cfg.slope != 1.0 else "", "-planar" if cfg.kind == "planar" else "")


def _subsets(present):
    """The full request first, then every other non-empty subset."""
    return [tuple(present)] + [s for r in range(1, len(present)) for s in itertools.combinations(present, r)]


# A Python exception of the host code under one request (the kind the matrix is there to find) is recorded and reported by the
# tests of that request; anything else raised while the device is in use ends every later device run of this module.
HOST_ERRORS = (AttributeError, TypeError, ValueError, IndexError, KeyError)
_device_error = []


def _on_device(fn):
    @functools.wraps(fn)
    def run(*a, **k):
        if _device_error:
            pytest.fail("not run: an earlier device run of this module raised %s" % _device_error[0])
        try:
            return fn(*a, **k)
        except HOST_ERRORS:
            raise
        except Exception as e:
            _device_error.append(repr(e)[:300])
            raise
    return run


def _kernels(calls):
    """The SphereConv kernel entry points among ``calls`` (not the host-only queries, not the geometry's table builders)."""
    return [n for n in calls if n.startswith("eml_sphere_") and n.endswith("_f32") and n != "eml_sphere_tap_table_f32"]


def _bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


@functools.lru_cache(None)
@_on_device
def _conv_runs(cfg):
    """Every request subset of one configuration, run once for all the tests below; everything returned lives on the CPU."""
    from emlight_amd.GenProjector import spherenet
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    B, C, O, H, W, stride = cfg.shape
    ho, wo = -(-H // stride), -(-W // stride)
    g = torch.Generator().manual_seed(1000 * CONFIGS.index(cfg) + C + O)
    cpu = {"x": torch.randn(B, C, H, W, generator=g),
           "weight": (torch.rand(O, C, 3, 3, generator=g) * 2 - 1) / (9 * C) ** 0.5 * 3 ** 0.5,
           "bias": torch.rand(O, generator=g) - 0.5 if cfg.bias else None,
           "residual": torch.randn(B, O, ho, wo, generator=g) if cfg.residual else None}
    gy_cpu = torch.randn(B, O, ho, wo, generator=g)
    present = [n for n in NAMES if cpu[n] is not None]
    cl = torch.channels_last
    out = {"inputs": cpu, "gy": gy_cpu, "present": present, "full": tuple(present), "runs": {}}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(SphereConv2D, "fused_min_bytes", 64 << 20)     # natural dispatch, whatever the A/B knobs of the environment say
        mp.setattr(SphereConv2D, "wgrad_workgroups", 1024)
        mp.setattr(SphereConv2D, "lowres", "off")
        for k, v in cfg.switches:
            mp.setattr(SphereConv2D, k, v)
        gy = gy_cpu.cuda().contiguous(memory_format=cl)
        geo = spherenet.sphere_geometry(H, W, stride, gy.device, cfg.kind)      # built before the recorder is in place
        out["transposed"] = geo.transposed_table() is not None
        plans, real_plan = [], spherenet._conv_plan

        def plan_spy(*a, **k):
            plans.append(real_plan(*a, **k))
            return plans[-1]
        mp.setattr(spherenet, "_conv_plan", plan_spy)
        seen = _spy_on_lib(mp)
        for subset in _subsets(present):
            t = {}
            for n in present:
                v = cpu[n].cuda()
                if n in ("x", "residual"):
                    t[n] = v.contiguous(memory_format=cl).requires_grad_(n in subset)
                else:                                       # parameters, as the networks hold them (a frozen one: no gradient)
                    t[n] = torch.nn.Parameter(v, requires_grad=n in subset)
            n0, p0 = len(seen), len(plans)
            try:
                if cfg.kind == "planar":
                    y = spherenet.planar_conv3x3(t["x"], t["weight"], t.get("bias"), stride, cfg.slope)
                else:
                    y = spherenet.sphere_conv(t["x"], t["weight"], t.get("bias"), stride, t.get("residual"), cfg.slope)
                n1 = len(seen)
                gs = torch.autograd.grad(y, [t[n] for n in subset], gy)
                torch.cuda.synchronize()
            except HOST_ERRORS as e:
                out["runs"][subset] = {"error": "%s: %s" % (type(e).__name__, e)}
                continue
            out["runs"][subset] = {"error": None, "y": y.detach().cpu(), "grads": {n: g_.detach().cpu() for n, g_ in zip(subset, gs)},
                                   "fwd": list(seen[n0:n1]), "bwd": list(seen[n1:]), "plan": plans[p0]}
    return out


def _errors(runs):
    return {s: r["error"] for s, r in runs.items() if r["error"]}


@functools.lru_cache(None)
def _oracle(cfg):
    """(exact, want): float64 output and gradients of the configuration, and the gradients for the full run's own mask (the same
    where there is no activation) -- computed once for every test that needs them."""
    r = _conv_runs(cfg)
    cpu = r["inputs"]
    args = (cfg.kind, cpu["x"], cpu["weight"], cpu["bias"], cfg.shape[5], cpu["residual"], cfg.slope, r["gy"])
    exact = oracle.grads(*args)
    return exact, exact if cfg.slope == 1.0 else oracle.grads_masked(*args, r["runs"][r["full"]]["y"])


def _expected_entry_points(cfg, plan, transposed):
    """The SphereConv entry points of a forward + backward under ``plan`` with every gradient wanted (``_plan_entry_points`` of
    tests/test_gpu_projector.py, extended by the forced footprint kernel, the one-pass narrow kernels and the geometry without a
    transposed tap table)."""
    B, C = cfg.shape[:2]
    if B == 0:
        return set()
    project = dict(cfg.switches).get("narrow_project", True)
    fwd = {"narrow": "conv_narrow_fwd2" if project else "conv_narrow_fwd", "small": "conv_small_fwd", "fused": "conv_fwd_fused_ex",
           "library": "im2col", "lowres": "conv_lowres"}[plan.fwd]
    dgrad = {"narrow": ["conv_narrow_dgrad2" if project and C <= 128 else "conv_narrow_dgrad"] if transposed else ["col2im"],
             "small": ["conv_small_da9", "col2im"], "fused": ["conv_dgrad_fused"] if transposed else ["col2im"],
             "library": ["col2im"], "lowres": ["conv_lowres"]}[plan.dgrad]
    wgrad = {"narrow": "conv_narrow_wgrad2" if project and transposed else "conv_narrow_wgrad", "small": "conv_small_wgrad",
             "fused": "conv_wgrad_fused", "library": "im2col"}[plan.wgrad]
    assert plan.keep == (plan.fwd == "library" and plan.wgrad == "library")
    return {"eml_sphere_%s_f32" % n for n in [fwd, wgrad] + dgrad}


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_every_request_subset_repeats_the_full_requests_bits(cfg):
    """(a) and (b): forward output and every requested gradient, bit for bit, under each of the up to 14 partial requests."""
    r = _conv_runs(cfg)
    assert not _errors(r["runs"]), _errors(r["runs"])
    full = r["runs"][r["full"]]
    assert len(r["runs"]) == 2 ** len(r["present"]) - 1
    bad = []
    for subset, run in r["runs"].items():
        if not _bits_equal(run["y"], full["y"]):
            bad.append((subset, "y", float((run["y"] - full["y"]).abs().max())))
        assert set(run["grads"]) == set(subset)
        for n, g in run["grads"].items():
            assert g.shape == r["inputs"][n].shape, (subset, n, g.shape)
            if not _bits_equal(g, full["grads"][n]):
                d = (g - full["grads"][n]).abs()
                to_bound = oracle.ratio_to_bound(g, _oracle(cfg)[1][n]) if g.numel() else 0.0
                bad.append((subset, "d" + n, "%d of %d elements, max |diff| %.3e of max |g| %.3e; %.3f of the bound of (d) against float64"
                            % (int((d > 0).sum()), d.numel(), float(d.max()), float(full["grads"][n].abs().max()), to_bound)))
    assert not bad, bad


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_no_kernel_runs_for_a_gradient_nobody_asked_for(cfg):
    """(c): the full request calls exactly its plan's entry points; a partial one none of the weight-gradient kernels (nor an
    im2col in its backward) without the weight, none of the input-gradient kernels (nor a second footprint launch) without x."""
    r = _conv_runs(cfg)
    assert not _errors(r["runs"]), _errors(r["runs"])
    full = r["runs"][r["full"]]
    ran = set(_kernels(full["fwd"] + full["bwd"]))
    assert ran == _expected_entry_points(cfg, full["plan"], r["transposed"]), (full["plan"], sorted(ran))
    for subset, run in r["runs"].items():
        calls = run["fwd"] + run["bwd"]
        assert run["plan"].fwd == full["plan"].fwd and _kernels(run["fwd"]) == _kernels(full["fwd"]), (subset, run["fwd"])
        # nothing the full request does not run either -- but the small family's bias gradient on its own, where the weight
        # gradient's kernel (which leaves it as a by-product) must not run
        alone = full["plan"].fwd == "small" and "bias" in subset and "weight" not in subset
        assert set(_kernels(calls)) - ran == ({SMALL_DBIAS} if alone else set()), (subset, sorted(set(_kernels(calls)) - ran))
        assert SMALL_DBIAS not in run["fwd"] and run["bwd"].count(SMALL_DBIAS) == int(alone), (subset, run["bwd"])
        if "weight" not in subset:
            assert run["plan"].wgrad is None and not run["plan"].keep, (subset, run["plan"])
            assert not set(calls) & set(WGRAD_ONLY), (subset, calls)
            assert "eml_sphere_im2col_f32" not in run["bwd"], (subset, run["bwd"])
        else:
            assert run["plan"].wgrad == full["plan"].wgrad, (subset, run["plan"])
        if "x" not in subset:
            assert run["plan"].dgrad is None, (subset, run["plan"])
            assert not set(calls) & set(DGRAD_ONLY), (subset, calls)
            assert calls.count("eml_sphere_conv_lowres_f32") == int(full["plan"].fwd == "lowres"), (subset, calls)
        else:
            assert run["plan"].dgrad == full["plan"].dgrad, (subset, run["plan"])


@pytest.mark.parametrize("cfg", NONEMPTY, ids=_id)
def test_full_request_vs_float64_oracle_elementwise(cfg):
    """(d): output and gradients of the full request against the tap-table restatement in float64, every element within rtol 1e-4
    + 1e-4 of the reference's largest entry; with an activation: gradients for the device output's own mask, and that mask differs
    from the exact one only where the exact output is within the output bound of zero."""
    r = _conv_runs(cfg)
    assert not r["runs"][r["full"]]["error"], r["runs"][r["full"]]["error"]
    full = r["runs"][r["full"]]
    exact, want = _oracle(cfg)
    ratios = {"y": oracle.ratio_to_bound(full["y"], exact["y"])}
    flips = 0
    if cfg.slope != 1.0:
        other = (full["y"] > 0) != (exact["y"] > 0)
        flips = int(other.sum())
        rtol, atol = oracle.bound(exact["y"])
        y64 = exact["y"][other].abs()
        assert bool((y64 <= atol + rtol * y64).all()), "the device's mask differs where |y64| is up to %.3e (bound %.3e)" % (float(y64.max()), atol)
    for n in r["present"]:
        ratios["d" + n] = oracle.ratio_to_bound(full["grads"][n], want[n])
    print("%s: %s of the bound; %d of %d outputs on the other side of zero"
          % (_id(cfg), ", ".join("%s %.3f" % kv for kv in ratios.items()), flips, full["y"].numel()))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("cfg", EMPTY, ids=_id)
def test_empty_batch_backward(cfg):
    """(e): the backward of an empty batch, under every subset: an empty dx, zero parameter gradients, no kernel."""
    r = _conv_runs(cfg)
    assert not _errors(r["runs"]), _errors(r["runs"])
    B, C, O, H, W, stride = cfg.shape
    for subset, run in r["runs"].items():
        assert run["y"].shape == (0, O, H // stride, W // stride)
        assert not _kernels(run["fwd"] + run["bwd"]), (subset, run["fwd"], run["bwd"])
        g = run["grads"]
        if "x" in subset:
            assert g["x"].shape == (0, C, H, W)
        if "weight" in subset:
            assert g["weight"].shape == (O, C, 3, 3) and not bool(g["weight"].any())
        if "bias" in subset:
            assert g["bias"].shape == (O,) and not bool(g["bias"].any())


def test_configurations_cover_every_plan_value_and_every_single_request():
    """The matrix names every kernel ``_conv_plan`` can choose for the forward and for either gradient, and each kernel path is run
    with x alone, the weight alone and the bias alone."""
    fwd, dgrad, wgrad = set(), set(), set()
    for cfg in CONFIGS:
        r = _conv_runs(cfg)
        paths = {s: run["plan"] for s, run in r["runs"].items() if not run["error"]}
        if cfg.shape[0] > 0:
            fwd |= {p.fwd for p in paths.values()}
            dgrad |= {p.dgrad for p in paths.values()}
            wgrad |= {p.wgrad for p in paths.values()}
    assert fwd == {"narrow", "small", "lowres", "fused", "library"}
    assert dgrad == {"narrow", "small", "lowres", "fused", "library", None}
    assert wgrad == {"narrow", "small", "fused", "library", None}
    assert {c.path for c in CONFIGS} == set(PATHS)
    for path in PATHS:
        with_bias = [c for c in CONFIGS if c.path == path and c.bias]
        assert with_bias, path
        for c in with_bias:
            present = [n for n in NAMES if n in ("x", "weight") or (n == "bias" and c.bias) or (n == "residual" and c.residual)]
            assert {("x",), ("weight",), ("bias",)} <= set(_subsets(present)), (path, c)
    assert any(c.residual for c in CONFIGS) and {c.slope for c in CONFIGS} == {1.0, 0.2, 0.0}


# ------------------------------------------------------------------------------------------ SPADE
# two shapes of test_spade_in_one_launch_vs_two_launches_and_stock_ops: (slope, B, C, nh, H, W, up2)
SPADE_SHAPES = [(0.2, 2, 64, 128, 16, 32, False), (0.2, 2, 128, 64, 12, 24, True)]
SPADE_INPUTS = ("x", "actv", "wg", "wb", "bg", "bb")
SPADE_SUBSETS = [SPADE_INPUTS, ("x",), ("actv",), ("wg", "wb", "bg", "bb"), ("wg",), ("wb", "bb"), ("bg", "bb"), ("x", "actv")]
BN_APPLY = ("eml_bn_bwd_apply_f32", "eml_bn_bwd_apply_up2_f32")


@functools.lru_cache(None)
@_on_device
def _spade_runs(shape, fuse, train):
    from emlight_amd.GenProjector.spherenet import SphereConv2D, spade_norm_modulate
    slope, B, C, nh, H, W, up2 = shape
    g = torch.Generator().manual_seed(5 + C)
    hx, wx = (H // 2, W // 2) if up2 else (H, W)
    cl = torch.channels_last
    cpu = {"x": torch.randn(B, C, hx, wx, generator=g) * 1.7 + 0.4, "actv": torch.randn(B, nh, H, W, generator=g),
           "wg": (torch.rand(C, nh, 3, 3, generator=g) * 2 - 1) / (3 * nh) ** 0.5,
           "wb": (torch.rand(C, nh, 3, 3, generator=g) * 2 - 1) / (3 * nh) ** 0.5,
           "bg": torch.rand(C, generator=g) * 0.6 - 0.3, "bb": torch.rand(C, generator=g) * 0.6 - 0.3}
    runs = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(SphereConv2D, "fused_min_bytes", 0)        # every layer on the fused kernels, whatever its size
        mp.setattr(SphereConv2D, "fuse_spade", fuse)
        mp.setattr(SphereConv2D, "lowres", "off")
        wy = torch.linspace(-1, 1, B * C * H * W, device="cuda").view(B, C, H, W)
        seen = _spy_on_lib(mp)
        for subset in SPADE_SUBSETS:
            bn = torch.nn.BatchNorm2d(C, affine=False).cuda().train(train)
            heads = (SphereConv2D(nh, C).cuda(), SphereConv2D(nh, C).cuda())
            with torch.no_grad():
                bn.running_mean.copy_(torch.linspace(-0.2, 0.3, C))
                bn.running_var.copy_(torch.linspace(0.5, 2.0, C))
                for m, w, b in zip(heads, ("wg", "wb"), ("bg", "bb")):
                    m.weight.copy_(cpu[w])
                    m.bias.copy_(cpu[b])
                    m.weight.requires_grad_(w in subset)
                    m.bias.requires_grad_(b in subset)
            t = {"x": cpu["x"].cuda().contiguous(memory_format=cl).requires_grad_("x" in subset),
                 "actv": cpu["actv"].cuda().contiguous(memory_format=cl).requires_grad_("actv" in subset),
                 "wg": heads[0].weight, "wb": heads[1].weight, "bg": heads[0].bias, "bb": heads[1].bias}
            n0 = len(seen)
            try:
                y = spade_norm_modulate(t["x"], bn, t["actv"], heads[0], heads[1], slope, None, up2)
                n1 = len(seen)
                gs = torch.autograd.grad(y, [t[n] for n in subset], wy)
                torch.cuda.synchronize()
            except HOST_ERRORS as e:
                runs[subset] = {"error": "%s: %s" % (type(e).__name__, e)}
                continue
            runs[subset] = {"error": None, "y": y.detach().cpu(), "grads": {n: g_.detach().cpu() for n, g_ in zip(subset, gs)},
                            "fwd": list(seen[n0:n1]), "bwd": list(seen[n1:]),
                            "stats": (bn.running_mean.cpu(), bn.running_var.cpu(), int(bn.num_batches_tracked))}
    return runs


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("shape", SPADE_SHAPES)
def test_spade_request_subsets_repeat_the_full_requests_bits(shape, fuse, train):
    """``spade_norm_modulate`` in one launch (``_SpadeConvModulateFn``) and in two (``_SpadeNormModulateFn`` + ``sphere_conv``):
    every partial request -- the heads alone with the guide map detached among them -- gives the full request's output and
    gradients bit for bit and leaves the same running statistics; BatchNorm's backward pass runs only where x wants a gradient.
    (The full request's parity with stock ops: test_spade_in_one_launch_vs_two_launches_and_stock_ops.)"""
    runs = _spade_runs(shape, fuse, train)
    assert not _errors(runs), _errors(runs)
    full = runs[SPADE_INPUTS]
    bad = []
    for subset, run in runs.items():
        assert ("eml_sphere_conv_spade_fwd_f32" in run["fwd"]) == fuse, (subset, run["fwd"])
        if not _bits_equal(run["y"], full["y"]):
            bad.append((subset, "y"))
        for n, g in run["grads"].items():
            if not _bits_equal(g, full["grads"][n]):
                d = (g - full["grads"][n]).abs()
                bad.append((subset, "d" + n, "%d of %d elements, max |diff| %.3e" % (int((d > 0).sum()), d.numel(), float(d.max()))))
        if "x" not in subset and set(run["bwd"]) & set(BN_APPLY):
            bad.append((subset, "BatchNorm's backward ran without a request for dx", sorted(set(run["bwd"]) & set(BN_APPLY))))
        if "x" in subset and not set(run["bwd"]) & set(BN_APPLY):
            bad.append((subset, "no BatchNorm backward"))
        for k in range(3):
            same = run["stats"][k] == full["stats"][k] if k == 2 else _bits_equal(run["stats"][k], full["stats"][k])
            if not same:
                bad.append((subset, "running statistics", k))
    assert not bad, bad
    assert full["stats"][2] == int(train)


# ------------------------------------------------------------------------------------------ the small family's bias gradient alone
# (B, H, W): one pixel short of a k-step and of a workgroup's 128; several workgroups with a partial last one; the persistent
# grid of 512 with more steps than two turns of its 2048 waves take (72864 pixels = 9108 steps), an odd number of turns
@pytest.mark.parametrize("O,slope", [(64, 1.0), (128, 0.2), (64, 0.0), (128, 1.0)])
@pytest.mark.parametrize("B,H,W", [(1, 3, 5), (3, 7, 11), (5, 33, 65), (33, 48, 46)])
@_on_device
def test_small_bias_gradient_alone_is_the_weight_gradient_kernels_column(B, H, W, O, slope):
    """``eml_sphere_conv_small_dbias_f32`` against the db of ``eml_sphere_conv_small_wgrad_f32`` on the same (dY, Y), bit for bit,
    and against the float64 column sum within the bound of (d)."""
    from emlight_amd import _lib
    from emlight_amd.GenProjector.spherenet import sphere_geometry
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    g = torch.Generator().manual_seed(B * 1000 + H + O)
    M = B * H * W
    x = torch.randn(B, H * W, 3, generator=g).cuda()
    gy, y = torch.randn(M, O, generator=g).cuda(), torch.randn(M, O, generator=g).cuda()
    geo = sphere_geometry(H, W, 1, x.device)
    n = L.eml_sphere_conv_small_wgrad_partial_floats(B, H * W, 3, O)
    part = torch.full((n,), float("nan"), device="cuda")
    dw2, db = torch.empty(O, 27, device="cuda"), torch.full((O,), float("nan"), device="cuda")
    ya = p(y) if slope != 1.0 else None
    _lib.check(L.eml_sphere_conv_small_wgrad_f32(p(x), p(geo.idx), p(geo.wgt), p(gy), ya, slope, p(part), p(dw2), p(db), B, H * W, H * W,
                                                 3, O, st), "eml_sphere_conv_small_wgrad_f32")
    part2 = torch.full((n,), float("nan"), device="cuda")
    alone = torch.full((O,), float("nan"), device="cuda")
    _lib.check(L.eml_sphere_conv_small_dbias_f32(p(gy), ya, slope, p(part2), p(alone), B, H * W, 3, O, st), "eml_sphere_conv_small_dbias_f32")
    torch.cuda.synchronize()
    masked = gy if slope == 1.0 else torch.where(y > 0, gy, gy * slope)
    want = masked.double().sum(0).cpu()
    print("M = %d: %.3f of the bound" % (M, oracle.ratio_to_bound(alone, want)))
    assert oracle.ratio_to_bound(alone, want) <= 1.0
    assert _bits_equal(alone.cpu(), db.cpu()), float((alone - db).abs().max())
    # one float per workgroup and channel of the scratch is used
    grid = min(512, (M + 127) // 128)
    assert bool(torch.isnan(part2[grid * O:]).all()) and not bool(torch.isnan(part2[:grid * O]).any())
