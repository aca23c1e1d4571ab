"""GPU: what the HIP backward paths write into the gradient buckets of ``emlight_amd._dist.GradientBuckets``, element by element.

Three producers write their weight gradients straight into the all-reduce buckets through ``_dist.grad_slot`` -- the encoder's
backward (every one of its 306 parameters), spectral norm's backward (``eml_spectral_norm_w2_bwd_f32``) and the SphereConv weight
gradient of a weight that is a parameter itself -- and autograd adopts the returned view as ``.grad``.  Single process, no process
group (``dp_active()`` is false: no collective is issued, but places, hooks, packing and ``finish()`` all run).

Every case: two ``deepcopy``-identical modules, A without a reducer and B with one, the same seeded inputs (another one per step)
and the same upstream gradient, three consecutive steps.  Before every backward of B its buckets are filled with NaN, so that "the
producer must write every element" is a deterministic check and not the caching allocator's luck (without a reducer the producers
write into ``torch.empty_like``, which tends to be last step's block with last step's plausible values).

a. ``.grad = None`` between the steps; on every step every ``.grad`` of B is its place in its bucket, no element of a place is NaN,
   every padding element between the places and after the last still is (places start every 32 floats: a store past ``numel``
   lands there), and ``torch.equal(gB, gA)``: the same kernels write to another address, 128-byte aligned like an allocation.
b. ``.grad`` kept and zeroed in place (``zero_grad(set_to_none=False)``) for steps 2 and 3, only the padding refilled: the same.
   ``.grad`` then IS the bucket view; a producer handed that place again overwrites it and autograd adds it to itself (twice the
   gradient, which is what this case showed before ``grad_slot`` refused the place of a parameter that has a ``.grad``).
c. a module applied twice in one forward: the second backward call gets no place, autograd sums, the gradient is A's.
d. once per producer, B's step-1 gradient against the reference and under the bound of that producer's own test:
   ``tests/test_gpu_densenet.py::test_backward_small_vs_oracle`` (``_grad_check``), ``tests/test_gpu_projector.py::
   test_fused_spectral_norm_vs_torch_hook`` (rtol 1e-4, atol 1e-5 of the largest entry), item d of
   ``tests/test_gpu_sphere_conv_requests.py`` (float64 restatement, ``ratio_to_bound``).
"""
import copy
import functools

import numpy as np
import pytest
import torch

from emlight_amd import _dist
from emlight_amd._dist import GradientBuckets

pytestmark = pytest.mark.gpu
NAN = float("nan")
STEPS = 3


# ------------------------------------------------------------------------------------------ the buckets under test
def _padding_masks(red):
    """Per bucket: True where an element of ``flat`` belongs to no parameter."""
    masks = []
    for b in red.buckets:
        m = torch.ones(b["flat"].numel(), dtype=torch.bool)
        for o, p in zip(b["offs"], b["params"]):
            assert o % 32 == 0
            m[o:o + p.numel()] = False
        masks.append(m.to(b["flat"].device))
    return masks


def _fill_nan(red, masks, only_padding):
    for b, m in zip(red.buckets, masks):
        if only_padding:
            b["flat"].masked_fill_(m, NAN)
        else:
            b["flat"].fill_(NAN)


def _place(red, p):
    """The view of ``p``'s place in its bucket."""
    b = red.buckets[red.where[id(p)]]
    return b["views"][[q is p for q in b["params"]].index(True)]


def _check_step(red, masks, named_b, want, what):
    """(a) for one finished step: places, NaN pattern, bit equality with A."""
    for name, p in named_b:
        assert p.grad is not None and p.grad.data_ptr() == _place(red, p).data_ptr() and p.grad.shape == p.shape, (what, name)
    for k, (b, m) in enumerate(zip(red.buckets, masks)):
        isnan = torch.isnan(b["flat"])
        if not torch.equal(isnan, m):
            unwritten = [(n, int(torch.isnan(p.grad).sum()), p.numel()) for n, p in named_b
                         if red.where[id(p)] == k and bool(torch.isnan(p.grad).any())]
            lost = int((m & ~isnan).sum())
            pytest.fail("%s, bucket %d: elements of a place left NaN (name, count, numel): %s; padding elements overwritten: %d "
                        "of %d" % (what, k, unwritten, lost, int(m.sum())))
    bad = []
    for (name, p), g in zip(named_b, want):
        if not torch.equal(p.grad, g):
            d = (p.grad - g).abs()
            ratio = float((p.grad.double().norm() / g.double().norm().clamp(min=1e-300)))
            bad.append((name, "%d of %d elements, max |diff| %.3e at max |g| %.3e, |gB| / |gA| = %.4f"
                        % (int((d > 0).sum()), d.numel(), float(d.max()), float(g.abs().max()), ratio)))
    assert not bad, (what, bad[:6], "%d tensors" % len(bad))


def _drive(base, run, cap_mb, keep):
    """Three steps of B = deepcopy(base) under a reducer against the recorded gradients of A.  ``run(module, step)`` -> loss."""
    want = _gradients_of_a(base, run)
    b = copy.deepcopy(base)
    params = list(b.parameters())
    named_b = list(b.named_parameters())
    red = GradientBuckets(params, world=2, cap_mb=cap_mb)
    try:
        assert len(red.buckets) == (len(params) if cap_mb == 0 else 1)
        masks = _padding_masks(red)
        for step in range(STEPS):
            if keep and step:
                b.zero_grad(set_to_none=False)
                for p in params:
                    assert p.grad is not None and not bool(p.grad.any())
                _fill_nan(red, masks, only_padding=True)
            else:
                for p in params:
                    p.grad = None
                _fill_nan(red, masks, only_padding=False)
            run(b, step).backward()
            red.finish()
            _check_step(red, masks, named_b, want[step], "step %d%s" % (step + 1, ", .grad kept" if keep and step else ""))
            assert red.next == 0 and not red.launched
    finally:
        for h in red.hooks:
            h.remove()


_A = {}


def _gradients_of_a(base, run):
    """A: a copy of ``base`` without a reducer, ``.grad = None`` between the steps -- run once per (base, run), shared by the
    cases of that pair and left unchanged."""
    key = (id(base), run)
    if key not in _A:
        a = copy.deepcopy(base)
        out = []
        for step in range(STEPS):
            for p in a.parameters():
                p.grad = None
            run(a, step).backward()
            out.append([p.grad.detach().clone() for p in a.parameters()])
        _A[key] = (base, out)      # (the base is held, so that its id is not reused)
    return _A[key][1]


def _spy_grad_slot(monkeypatch):
    """Every ``grad_slot`` call of the producers (they look it up in ``_dist`` when they run): (asked by pointer?, got a place?)."""
    calls, real = [], _dist.grad_slot

    def spy(param=None, ptr=None):
        r = real(param, ptr)
        calls.append((ptr if param is None else param.data_ptr(), r is not None))
        return r
    monkeypatch.setattr(_dist, "grad_slot", spy)
    return calls


# ------------------------------------------------------------------------------------------ the encoder
KEYS = ("distribution", "intensity", "rgb_ratio", "ambient")
ENCODER_SHAPES = [((32, 32), 3), ((64, 96), 2)]


@functools.lru_cache(None)
def _encoder_case(crop_hw, B):
    """(the oracle, the HIP network with the same seeded weights -- never run itself --, run(module, step))."""
    from tests.test_gpu_densenet import _pair
    ref, net = _pair(32, crop_hw, seed=5)
    ref.train(), net.train()
    g = np.random.default_rng([4, B])        # the inputs of test_backward_small_vs_oracle first, then two more crops
    xs = [torch.from_numpy(g.random((B, 3) + crop_hw, dtype=np.float32))]
    w = {k: torch.from_numpy(g.standard_normal(s).astype(np.float32))
         for k, s in (("distribution", (B, 32)), ("intensity", (B, 1)), ("rgb_ratio", (B, 3)), ("ambient", (B, 3)))}
    xs += [torch.from_numpy(g.random((B, 3) + crop_hw, dtype=np.float32)) for _ in range(STEPS - 1)]
    xg, wg = [x.cuda() for x in xs], {k: v.cuda() for k, v in w.items()}

    def run(m, step):      # a fixed seeded linear functional of the four outputs
        out = m(xg[step])
        return sum((out[k] * wg[k]).sum() for k in KEYS)
    return ref, net, run, xs[0], w


@pytest.mark.parametrize("keep", [False, True], ids=["grad-none", "grad-kept"])
@pytest.mark.parametrize("cap_mb", [0, 64], ids=["bucket-per-parameter", "one-bucket"])
@pytest.mark.parametrize("crop_hw,B", ENCODER_SHAPES)
def test_encoder_backward_writes_its_bucket_places(crop_hw, B, cap_mb, keep):
    """(a) and (b) for ``run_backward`` (RegressionNetwork/dense_engine_bwd.py): the encoder's 306 parameters written in place by the
    kernels, the ten of the heads packed by the reducer."""
    from emlight_amd.RegressionNetwork.dense_engine import HipDenseEncoder
    _, net, run, _, _ = _encoder_case(crop_hw, B)
    assert len(HipDenseEncoder(net).param_list()) == 306 and len(list(net.parameters())) == 316
    _drive(net, run, cap_mb, keep)


def test_encoder_bucket_gradient_vs_oracle():
    """(d): B's gradient of the step of ``test_backward_small_vs_oracle`` (64 x 96, B = 2), written into one bucket, under that
    test's ``_grad_check``."""
    from tests.test_gpu_densenet import _grad_check
    ref, net, run, x0, w = _encoder_case((64, 96), 2)
    ref = copy.deepcopy(ref)
    po = ref(x0)
    sum((po[k] * w[k]).sum() for k in KEYS).backward()
    b = copy.deepcopy(net)
    red = GradientBuckets(list(b.parameters()), world=2, cap_mb=64)
    try:
        red.buckets[0]["flat"].fill_(NAN)
        run(b, 0).backward()
        red.finish()
        _grad_check(b, ref)
    finally:
        for h in red.hooks:
            h.remove()


# ------------------------------------------------------------------------------------------ spectral norm
# (O, C): the vector re-layout; C not a multiple of 4: the scalar one; two channel chunks of 256, the second of 4 channels
SPECTRAL_SHAPES = [(64, 32), (40, 6), (8, 260)]


@functools.lru_cache(None)
def _spectral_case(O, C):
    from emlight_amd.GenProjector.spherenet import SphereConv2D, fused_spectral_norm
    torch.manual_seed(O + C)
    conv = SphereConv2D(C, O).cuda()
    with torch.no_grad():
        conv.weight.normal_(0, 0.05)
        conv.bias.uniform_(-0.5, 0.5)
    g = torch.Generator().manual_seed(7 * O + C)
    xs = [torch.randn(2, C, 8, 16, generator=g).cuda() for _ in range(STEPS + 1)]
    gy = torch.randn(2, O, 8, 16, generator=g).cuda()
    base = fused_spectral_norm(copy.deepcopy(conv)).train()

    def run(m, step):
        return (m(xs[step]) * gy).sum()

    def run_twice(m, step):
        return (m(xs[step]) * gy).sum() + 0.5 * (m(xs[step + 1]) * gy).sum()
    return conv, base, run, run_twice


@pytest.mark.parametrize("keep", [False, True], ids=["grad-none", "grad-kept"])
@pytest.mark.parametrize("cap_mb", [0, 64], ids=["bucket-per-parameter", "one-bucket"])
@pytest.mark.parametrize("O,C", SPECTRAL_SHAPES)
def test_spectral_norm_backward_writes_its_bucket_place(O, C, cap_mb, keep, monkeypatch):
    """(a) and (b) for ``_SpectralW2Fn.backward``: ``weight_orig``'s gradient by ``eml_spectral_norm_w2_bwd_f32`` in place, the
    bias packed."""
    _, base, run, _ = _spectral_case(O, C)
    _gradients_of_a(base, run)                 # (A's calls, which get no place, stay out of the record)
    calls = _spy_grad_slot(monkeypatch)
    _drive(base, run, cap_mb, keep)
    assert [got for _, got in calls] == ([True, False, False] if keep else [True] * STEPS)   # a place while weight_orig has no .grad


def test_spectral_norm_module_applied_twice(monkeypatch):
    """(c): two ``_SpectralW2Fn`` nodes for one ``weight_orig``: one place, one tensor of its own, their sum is A's."""
    _, base, _, run_twice = _spectral_case(64, 32)
    _gradients_of_a(base, run_twice)
    calls = _spy_grad_slot(monkeypatch)
    _drive(base, run_twice, 64, False)
    assert [got for _, got in calls] == [True, False] * STEPS


def test_spectral_norm_bucket_gradient_vs_torch_hook():
    """(d): the reference and the bound of ``test_fused_spectral_norm_vs_torch_hook`` -- torch's own hook on the same
    ``weight_orig`` / ``u`` / ``v``, rtol 1e-4 and atol 1e-5 of the largest entry -- for the gradient in the bucket."""
    from emlight_amd.GenProjector.spherenet import fused_spectral_norm
    for O, C in SPECTRAL_SHAPES:
        conv, _, run, _ = _spectral_case(O, C)
        ref = torch.nn.utils.spectral_norm(copy.deepcopy(conv)).train()
        hip = fused_spectral_norm(copy.deepcopy(conv)).train()
        hip.load_state_dict(ref.state_dict())
        red = GradientBuckets(list(hip.parameters()), world=2, cap_mb=64)
        try:
            red.buckets[0]["flat"].fill_(NAN)
            run(ref, 0).backward()
            run(hip, 0).backward()
            red.finish()
            for name in ("weight_orig", "bias"):
                want, got = getattr(ref, name).grad, getattr(hip, name).grad
                assert got.data_ptr() == _place(red, getattr(hip, name)).data_ptr()
                np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-5 * float(want.abs().max()),
                                           err_msg="%s of (%d, %d)" % (name, O, C))
        finally:
            for h in red.hooks:
                h.remove()


# ------------------------------------------------------------------------------------------ SphereConv, a weight that is a parameter
# (B, Cin, Cout, H, W, stride): the "small", "narrow" and "library" rows of tests/test_gpu_sphere_conv_requests.py
CONV_SHAPES = [(2, 3, 64, 8, 16, 1), (2, 64, 3, 16, 32, 1), (2, 16, 8, 8, 16, 1)]
CONV_WGRAD = {(2, 3, 64, 8, 16, 1): "small", (2, 64, 3, 16, 32, 1): "narrow", (2, 16, 8, 8, 16, 1): "library"}


@pytest.fixture
def natural_dispatch(monkeypatch):
    """The dispatch of tests/test_gpu_sphere_conv_requests.py, whatever the A/B knobs of the environment say."""
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    monkeypatch.setattr(SphereConv2D, "fused_min_bytes", 64 << 20)
    monkeypatch.setattr(SphereConv2D, "wgrad_workgroups", 1024)
    monkeypatch.setattr(SphereConv2D, "lowres", "off")
    monkeypatch.setattr(SphereConv2D, "narrow_project", True)


@functools.lru_cache(None)
def _conv_case(shape):
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    B, C, O, H, W, stride = shape
    g = torch.Generator().manual_seed(31 * C + O)
    base = SphereConv2D(C, O, stride).cuda()
    cpu = {"weight": (torch.rand(O, C, 3, 3, generator=g) * 2 - 1) / (9 * C) ** 0.5 * 3 ** 0.5, "bias": torch.rand(O, generator=g) - 0.5,
           "xs": [torch.randn(B, C, H, W, generator=g) for _ in range(STEPS + 1)],
           "gy": torch.randn(B, O, -(-H // stride), -(-W // stride), generator=g)}
    with torch.no_grad():
        base.weight.copy_(cpu["weight"])
        base.bias.copy_(cpu["bias"])
    cl = torch.channels_last
    xs, gy = [x.cuda().contiguous(memory_format=cl) for x in cpu["xs"]], cpu["gy"].cuda().contiguous(memory_format=cl)

    def run(m, step):
        return (m(xs[step]) * gy).sum()

    def run_twice(m, step):
        return (m(xs[step]) * gy).sum() + 0.5 * (m(xs[step + 1]) * gy).sum()
    return cpu, base, run, run_twice


@pytest.mark.parametrize("keep", [False, True], ids=["grad-none", "grad-kept"])
@pytest.mark.parametrize("cap_mb", [0, 64], ids=["bucket-per-parameter", "one-bucket"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sphere_conv_leaf_weight_gradient_lands_in_its_bucket_place(shape, cap_mb, keep, natural_dispatch, monkeypatch):
    """(a) and (b) for ``_sphere_conv_backward``: the weight gradient's re-layout to the parameter's own order lands in the place,
    the bias gradient is packed."""
    from emlight_amd.GenProjector import spherenet
    _, base, run, _ = _conv_case(shape)
    _gradients_of_a(base, run)
    plans, real_plan = [], spherenet._conv_plan
    monkeypatch.setattr(spherenet, "_conv_plan", lambda *a, **k: (plans.append(real_plan(*a, **k)), plans[-1])[1])
    calls = _spy_grad_slot(monkeypatch)
    _drive(base, run, cap_mb, keep)
    assert len(plans) == STEPS and {p.wgrad for p in plans} == {CONV_WGRAD[shape]}, plans[:1]
    assert [got for _, got in calls] == ([True, False, False] if keep else [True] * STEPS)


def test_sphere_conv_module_applied_twice(natural_dispatch, monkeypatch):
    """(c): the second backward call of one weight gets no place."""
    _, base, _, run_twice = _conv_case(CONV_SHAPES[0])
    _gradients_of_a(base, run_twice)
    calls = _spy_grad_slot(monkeypatch)
    _drive(base, run_twice, 64, False)
    assert [got for _, got in calls] == [True, False] * STEPS


def test_sphere_conv_bucket_gradient_vs_float64_oracle(natural_dispatch):
    """(d): item d of tests/test_gpu_sphere_conv_requests.py -- the float64 restatement from the tap table, every element within
    rtol 1e-4 + 1e-4 of the reference's largest entry -- for the weight and bias gradients in the bucket."""
    from tests import sphere_conv_oracle as oracle
    for shape in CONV_SHAPES:
        cpu, base, run, _ = _conv_case(shape)
        want = oracle.grads("sphere", cpu["xs"][0], cpu["weight"], cpu["bias"], shape[5], None, 1.0, cpu["gy"])
        b = copy.deepcopy(base)
        red = GradientBuckets(list(b.parameters()), world=2, cap_mb=64)
        try:
            red.buckets[0]["flat"].fill_(NAN)
            run(b, 0).backward()
            red.finish()
            ratios = {n: oracle.ratio_to_bound(getattr(b, n).grad, want[n]) for n in ("weight", "bias")}
            print("%s: %s of the bound" % ("x".join(map(str, shape)), ", ".join("d%s %.3f" % kv for kv in ratios.items())))
            assert max(ratios.values()) <= 1.0, (shape, ratios)
        finally:
            for h in red.hooks:
                h.remove()
