"""``emlight_amd._dist.GradientBuckets`` on the CPU, without a process group (the collectives themselves: tests/test_ddp_gloo.py
with two gloo ranks, tests/test_gpu_ddp_two_ranks.py): packing, bucket views as ``.grad``, parameters without a gradient, and
``grad_slot`` -- a producer writing straight into its parameter's place in the bucket."""
import copy

import torch

from emlight_amd import _dist
from emlight_amd._dist import GradientBuckets, grad_slot


def _inside(t, flat):
    return flat.data_ptr() <= t.data_ptr() < flat.data_ptr() + flat.numel() * flat.element_size()


def test_buckets_pack_views_and_unused_parameters():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4))
    spare = torch.nn.Linear(4, 4)                      # registered with the reducer, never used in the forward
    ref = copy.deepcopy(net)
    params = list(net.parameters()) + list(spare.parameters())
    red = GradientBuckets(params, world=2, cap_mb=0)   # cap 0: one bucket per parameter -- exercises the in-order launch
    assert len(red.buckets) == len(params) and red.describe()["bytes"] == sum(4 * p.numel() for p in params)
    assert [b["params"][0] is p for b, p in zip(red.buckets, reversed(params))] == [True] * len(params)   # reverse registration order
    x = torch.randn(5, 8)
    for it in range(2):                                # the second iteration reuses the buckets
        for p in params:
            p.grad = None
        net(x).square().sum().backward()
        assert red.next == 0 or red.next <= len(params)
        red.finish()
        ref.zero_grad(set_to_none=True)
        ref(x).square().sum().backward()
        for p, q in zip(net.parameters(), ref.parameters()):
            b = red.buckets[red.where[id(p)]]
            assert _inside(p.grad, b["flat"]) and p.grad.shape == p.shape
            torch.testing.assert_close(p.grad, q.grad, rtol=0, atol=0)
        for p in spare.parameters():                   # no gradient in this backward: zeros, in the bucket
            assert _inside(p.grad, red.buckets[red.where[id(p)]]["flat"]) and float(p.grad.abs().max()) == 0.0
        assert red.next == 0 and not red.launched and all(b["pending"] == len(b["params"]) for b in red.buckets)


class _Lin(torch.autograd.Function):
    """x @ w.T whose backward asks for the weight gradient's place in the bucket, like the HIP producers do."""
    got = []

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        ctx.wptr = w.data_ptr()
        return x @ w.t()

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gw = g.t() @ x
        slot = grad_slot(ptr=ctx.wptr)
        _Lin.got.append(slot is not None)
        if slot is not None:
            slot.copy_(gw)
            gw = slot
        return g @ w, gw


def test_grad_slot_is_adopted_without_packing_and_refused_the_second_time():
    torch.manual_seed(1)
    w = torch.nn.Parameter(torch.randn(6, 8))
    w2 = torch.nn.Parameter(torch.randn(6, 8))
    red = GradientBuckets([w, w2], world=2, cap_mb=64)
    flat = red.buckets[0]["flat"]
    x = torch.randn(3, 8)
    packed = []
    inner = torch._foreach_copy_
    try:
        torch._foreach_copy_ = lambda dst, src, *a, **k: (packed.append(len(src)), inner(dst, src, *a, **k))[1]
        _Lin.got.clear()
        (_Lin.apply(x, w).sum() + _Lin.apply(x, w2).square().sum()).backward()
        assert _Lin.got == [True, True]
        assert _inside(w.grad, flat) and _inside(w2.grad, flat)      # autograd adopted the returned views
        red.finish()
        assert packed == []                                           # nothing left to pack
        torch.testing.assert_close(w.grad, torch.ones(3, 6).t() @ x, rtol=0, atol=0)
        # a parameter used twice in one forward: the second backward call gets no place (autograd has to sum two tensors)
        w.grad = w2.grad = None
        _Lin.got.clear()
        (_Lin.apply(x, w).sum() + _Lin.apply(2 * x, w).sum() + _Lin.apply(x, w2).sum()).backward()
        assert sorted(_Lin.got) == [False, True, True]
        red.finish()
        assert _inside(w.grad, flat)
        torch.testing.assert_close(w.grad, 3 * (torch.ones(3, 6).t() @ x), rtol=1e-6, atol=1e-6)
    finally:
        torch._foreach_copy_ = inner
    assert grad_slot(ptr=12345) is None and grad_slot(torch.nn.Parameter(torch.zeros(2))) is None
    with torch.enable_grad():
        assert grad_slot(w) is None                                   # a graph-building backward gets no place


def test_places_of_a_deleted_reducer_are_not_handed_out():
    import gc
    w = torch.nn.Parameter(torch.randn(4, 4))
    red = GradientBuckets([w], world=2)
    with torch.no_grad():
        assert grad_slot(w) is not None
    ptr = w.data_ptr()
    for h in red.hooks:
        h.remove()
    del red
    gc.collect()
    with torch.no_grad():
        assert grad_slot(w) is None and grad_slot(ptr=ptr) is None
    GradientBuckets([torch.nn.Parameter(torch.zeros(1))], world=2)    # construction purges the dead entries
    assert ("ptr", ptr) not in _dist._SLOTS


# ---- a ``.grad`` that is kept over the step, and a second backward before finish() ------------------------------------------
# After a step ``.grad`` IS the bucket view.  A producer that were handed the same place again would overwrite it and autograd
# would then add the place to itself: twice the gradient, silently.  ``grad_slot`` therefore hands out nothing while a ``.grad``
# exists, and the reducer refuses a second backward before ``finish()``.

class _Net(torch.nn.Module):
    """Two ``_Lin`` producers and a plain ``nn.Linear`` (weight and bias: no producer) in one reducer."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(6, 8))
        self.w2 = torch.nn.Parameter(torch.randn(6, 8))
        self.head = torch.nn.Linear(6, 4)

    def forward(self, x, twice=False):
        h = _Lin.apply(x, self.w) + _Lin.apply(x, self.w2).square()
        if twice:
            h = h + _Lin.apply(2 * x + 1, self.w)
        return self.head(torch.tanh(h)).square().sum()


def _net_pair(seed, cap_mb=64):
    """B with a reducer, A -- a private copy -- without: the same ``_Lin`` products, which get no place for A's parameters."""
    torch.manual_seed(seed)
    b = _Net()
    a = copy.deepcopy(b)
    return a, b, GradientBuckets(list(b.parameters()), world=2, cap_mb=cap_mb, name="toy")


class _spy_foreach_copy:
    def __enter__(self):
        self.packed, self.inner = [], torch._foreach_copy_
        torch._foreach_copy_ = lambda dst, src, *a, **k: (self.packed.append(len(src)), self.inner(dst, src, *a, **k))[1]
        return self.packed

    def __exit__(self, *exc):
        torch._foreach_copy_ = self.inner


def _same_grads(a, b, red):
    for (n, p), q in zip(b.named_parameters(), a.parameters()):
        assert _inside(p.grad, red.buckets[red.where[id(p)]]["flat"]), n    # still the bucket view
        torch.testing.assert_close(p.grad, q.grad, rtol=0, atol=0, msg=lambda m, n=n: "%s: %s" % (n, m))


def _clean(red):
    return red.next == 0 and not red.launched and all(b["pending"] == len(b["params"]) and not b["taken"] for b in red.buckets)


def test_grad_kept_and_zeroed_in_place_is_not_doubled():
    for cap_mb in (64, 0):
        a, b, red = _net_pair(2, cap_mb)
        opt_a, opt_b = torch.optim.SGD(a.parameters(), lr=0.01), torch.optim.SGD(b.parameters(), lr=0.01)
        xs = torch.randn(3, 5, 8)
        with _spy_foreach_copy() as packed:
            for step in range(3):
                opt_a.zero_grad(set_to_none=False)
                opt_b.zero_grad(set_to_none=False)
                _Lin.got.clear()
                del packed[:]
                a(xs[step]).backward()
                assert _Lin.got == [False, False]                     # A has no reducer
                _Lin.got.clear()
                b(xs[step]).backward()
                red.finish()
                # the first step finds no .grad: both producers get their places, head.weight / head.bias are packed; from then
                # on .grad is the bucket view: no place is handed out, autograd adds into the view, nothing is packed
                assert _Lin.got == ([True, True] if step == 0 else [False, False])
                assert sum(packed) == (2 if step == 0 else 0)
                _same_grads(a, b, red)
                assert _clean(red)
                opt_a.step()
                opt_b.step()
        for h in red.hooks:
            h.remove()


def test_grad_never_cleared_accumulates_like_torch():
    a, b, red = _net_pair(3)
    xs = torch.randn(3, 5, 8)                                         # another input per step: 2 * g1 is not g1 + g2
    single = []
    for step in range(3):
        c = copy.deepcopy(a)
        c.zero_grad(set_to_none=True)
        c(xs[step]).backward()
        single.append([q.grad.clone() for q in c.parameters()])
        a(xs[step]).backward()
        b(xs[step]).backward()
        red.finish()
        _same_grads(a, b, red)
        want = [g.clone() for g in single[0]]                         # g1, then g1 + g2, then (g1 + g2) + g3
        for gs in single[1:]:
            want = [w + g for w, g in zip(want, gs)]
        for (n, p), w in zip(b.named_parameters(), want):
            torch.testing.assert_close(p.grad, w, rtol=0, atol=0, msg=lambda m, n=n: "%s, step %d: %s" % (n, step, m))
    for h in red.hooks:
        h.remove()


def test_second_backward_before_finish_is_refused():
    import pytest
    for cap_mb in (64, 0):
        a, b, red = _net_pair(4, cap_mb)
        xs = torch.randn(3, 5, 8)
        b(xs[0]).backward()
        launched = len(red.launched)
        assert launched == len(red.buckets)
        with pytest.raises(RuntimeError, match=r"'toy'.*a second backward before finish\(\)"):
            b(xs[1]).backward()
        assert len(red.launched) == launched                          # nothing was launched again
        assert all(x["pending"] >= 0 for x in red.buckets)
        red.finish()
        assert _clean(red)
        for p in b.parameters():
            p.grad = None
        a(xs[2]).backward()
        _Lin.got.clear()
        b(xs[2]).backward()
        red.finish()
        assert _Lin.got == [True, True]
        _same_grads(a, b, red)
        assert _clean(red)
        for h in red.hooks:
            h.remove()


def test_parameter_used_twice_with_grad_kept():
    a, b, red = _net_pair(5)
    xs = torch.randn(2, 5, 8)
    for step in range(2):
        a.zero_grad(set_to_none=False)
        b.zero_grad(set_to_none=False)
        a(xs[step], twice=True).backward()
        _Lin.got.clear()
        b(xs[step], twice=True).backward()
        red.finish()
        assert sorted(_Lin.got) == ([False, True, True] if step == 0 else [False, False, False])
        if step:                                                      # (step 0: the existing test of a module used twice)
            _same_grads(a, b, red)
    for h in red.hooks:
        h.remove()


def test_mixed_state_in_one_bucket():
    a, b, red = _net_pair(6)
    assert len(red.buckets) == 1
    bk = red.buckets[0]
    xs = torch.randn(2, 5, 8)
    a(xs[0]).backward()
    b(xs[0]).backward()
    red.finish()
    a.w.grad = b.w.grad = None                                        # w: cleared; its neighbour w2 and the head: kept
    for net in (a, b):
        for p in (net.w2, net.head.weight, net.head.bias):
            p.grad.zero_()
    a(xs[1]).backward()
    _Lin.got.clear()
    b(xs[1]).backward()
    assert sorted(_Lin.got) == [False, True]
    assert bk["taken"] == {[p is b.w for p in bk["params"]].index(True)}   # w2's place was not handed out
    with torch.no_grad():
        assert grad_slot(b.w2) is None and grad_slot(ptr=b.w2.data_ptr()) is None   # by object and by address
    red.finish()
    _same_grads(a, b, red)
    for h in red.hooks:
        h.remove()
