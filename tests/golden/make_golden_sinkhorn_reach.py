#!/usr/bin/env python
"""Generate tests/golden/sinkhorn_reach.npz: the REFERENCE's unbalanced Sinkhorn (SamplesLoss(reach=...)) on the CPU, f32.

Run only in the build container, where the reference checkout exists (see make_golden.py):

    python tests/golden/make_golden_sinkhorn_reach.py

The reference modules run unchanged; only ``reach`` is set on the criterion (``ref_samples_loss`` builds it with
``reach=None``).  ``scaling_parameters`` then sets ``rho = reach**p`` (``sinkhorn_divergence.py:35``) and ``sinkhorn_loop``
damps every softmin by ``dampening(eps, rho)`` (``:43-44, 78-107``).  Stored per case: x, y, loss, grad_x, eps_s, diameter,
the final duals, lam (the reference's own ``dampening`` of every schedule entry), blur and reach; the GMLight case also
stores its depth.  Every case is also run balanced on the same inputs, and the script asserts that at least one of loss,
duals or grad_x moves by more than 10x the GPU test's bound for it: a kernel that ignored the dampening would fail there.
Arrays only; the GPU tests read only the ``.npz``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference location, shims and the Sinkhorn input recipes)

# name, kind, B, N, blur, reach (gmloss: the GMLight criterion with a per-anchor depth)
REACH_CASES = [
    ("n96_softmax_blur025_r05", "softmax", 4, 96, .025, .05),
    ("n128_sparse_r1", "sparse", 4, 128, .05, .1),         # BASELINE cfg2 shape
    ("n256_sparse_r05", "sparse", 2, 256, .05, .05),       # BASELINE cfg5 shape
    ("n256_sparse_r3", "sparse", 2, 256, .05, .3),
    ("n50_ragged_r1", "softmax", 2, 50, .05, .1),          # ragged N
    ("n96_tiny_r05", "tiny", 2, 96, .05, .05),             # diameter < blur: a two-entry schedule
    ("n96_logits_r1", "logits", 3, 96, .025, 1.0),         # many eps steps, lam_first << 1
    ("gmloss_b3_r1", "gmloss", 3, 128, .05, .1),
]
SEED = 31

# the GPU test's bounds (tests/test_gpu_sinkhorn_reach.py, those of test_gpu_sinkhorn.py::test_golden_cases)
LOSS_ATOL, DUALS_REL, GRAD_RTOL = 1e-6, 2e-6, 1e-4


def _run(crit, x_np, y_np, extra=()):
    """loss, grad_x and the internals (schedule, rho, final duals) of one reference call."""
    import geomloss.samples_loss as gsl
    import gmloss.samples_loss as msl
    B, n = x_np.shape
    x = torch.from_numpy(x_np).view(B, n, 1).requires_grad_(True)
    y = torch.from_numpy(y_np).view(B, n, 1)
    cap = {}

    def wrap(orig_sp, orig_cost):   # each module's own scaling_parameters / sinkhorn_cost, observed
        def sp(*a, **k):
            r = orig_sp(*a, **k)
            cap["diameter"], cap["eps_s"], cap["rho"] = r[0], list(r[2]), r[3]
            return r

        def sc(eps, rho, a, b, a_x, b_y, a_y, b_x):
            cap["duals"] = np.stack([t.detach().numpy().copy() for t in (a_x, b_y, a_y, b_x)])
            return orig_cost(eps, rho, a, b, a_x, b_y, a_y, b_x)
        return sp, sc

    mods = (gsl, msl)
    saved = [(m.scaling_parameters, m.sinkhorn_cost) for m in mods]
    for m, (a, b) in zip(mods, saved):
        m.scaling_parameters, m.sinkhorn_cost = wrap(a, b)
    try:
        loss = crit(x, y, *extra)
    finally:
        for m, (a, b) in zip(mods, saved):
            m.scaling_parameters, m.sinkhorn_cost = a, b
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy().reshape(B, n), cap


def gen_sinkhorn_reach():
    geomloss, gutils = mg.ref_geomloss()
    import gmloss  # noqa: the reference package (same directory as geomloss)
    from geomloss import sinkhorn_divergence as sd
    out = {}
    for name, kind, B, n, blur, reach in REACH_CASES:
        extra = ()
        if kind == "gmloss":
            x_np, y_np, depth = mg.gmloss_inputs(B, SEED)
            extra = (depth,)
            out[name + "/depth"] = depth

            def make():
                return gmloss.SamplesLoss("sinkhorn", p=2, blur=blur, batchsize=B)
        else:
            x_np, y_np = mg.sinkhorn_inputs(kind, B, n, SEED)

            def make():
                return mg.ref_samples_loss(geomloss, gutils, n, B, blur)
        crit = make()
        crit.reach = reach
        loss, gx, cap = _run(crit, x_np, y_np, extra)
        assert cap["rho"] == reach ** 2
        lam = [sd.dampening(e, cap["rho"]) for e in cap["eps_s"]]
        bal_loss, bal_gx, bal_cap = _run(make(), x_np, y_np, extra)
        assert bal_cap["rho"] is None and bal_cap["eps_s"] == cap["eps_s"]
        # how far the balanced numbers are from the damped ones, in units of the GPU test's bound
        loss_bound = LOSS_ATOL * max(1.0, float(np.abs(loss).max()) / 1e-4)
        duals_bound = DUALS_REL * max(1.0, float(np.abs(cap["duals"]).max()))
        grad_bound = GRAD_RTOL * float(np.abs(gx).max()) + GRAD_RTOL * np.abs(gx)
        sep = {"loss": float(np.abs(loss - bal_loss).max()) / loss_bound,
               "duals": float(np.abs(cap["duals"] - bal_cap["duals"]).max()) / duals_bound,
               "grad_x": float((np.abs(gx - bal_gx) / grad_bound).max())}
        assert max(sep.values()) > 10.0, (name, sep)
        out[name + "/x"], out[name + "/y"] = x_np, y_np
        out[name + "/loss"], out[name + "/grad_x"] = loss, gx
        out[name + "/eps_s"] = np.asarray(cap["eps_s"], dtype=np.float64)
        out[name + "/lam"] = np.asarray(lam, dtype=np.float64)
        out[name + "/diameter"] = np.float64(cap["diameter"])
        out[name + "/duals"] = cap["duals"]
        out[name + "/blur"], out[name + "/reach"] = np.float64(blur), np.float64(reach)
        print("sinkhorn reach", name, "n_eps", len(lam), "lam %.4g .. %.4g" % (lam[0], lam[-1]),
              "loss0 %.4e (balanced %.4e)" % (loss[0], bal_loss[0]),
              "balanced vs damped, in bounds: " + " ".join("%s %.3g" % kv for kv in sep.items()))
    np.savez_compressed(os.path.join(HERE, "sinkhorn_reach.npz"), **out)


if __name__ == "__main__":
    mg.install_shims()
    gen_sinkhorn_reach()
