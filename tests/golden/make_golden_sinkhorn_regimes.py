#!/usr/bin/env python
"""Generate tests/golden/sinkhorn_regimes.npz: the REFERENCE's Sinkhorn loss away from its default constructor arguments
(p, scaling, blur) and away from simplex inputs, on the CPU, f32.

Run only in the build container, where the reference checkout exists (see make_golden.py):

    python tests/golden/make_golden_sinkhorn_regimes.py

The reference modules run unchanged; ``p``, ``scaling``, ``blur`` and ``reach`` are set on the criterion that
``ref_samples_loss`` builds (it passes them to ``sinkhorn_tensorized``, ``samples_loss.py:35-46``).  The weighted case calls
``sinkhorn_tensorized(alpha, x, beta, y, ...)`` directly, as make_golden_sinkhorn_dim.py does (the reference's own
four-argument ``forward`` fails to unpack).  Stored per case: x, y, (alpha, beta), loss, grad_x, the captured ``eps_s``, the
diameter, the four final duals, p, scaling, blur and reach (0: balanced).  Arrays only; the tests read only the ``.npz``.

``SETTINGS``, ``REGIMES`` and ``regime_inputs`` are also what tests/test_gpu_sinkhorn_regimes.py runs the HIP kernels on
(importing this module needs neither the reference nor make_golden's shims).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (p, scaling, blur)
SETTINGS = {"S1": (2, .9, .05), "S2": (1, .5, .05), "S3": (3, .7, .10), "S4": (2, .3, .05), "S5": (2, .8, .01)}
REGIMES = ("softmax", "logits", "x30", "offset")
SEED = 53

# name, setting, regime, D, reach (0: balanced), weighted
REGIME_CASES = [("S1_logits", "S1", "logits", 1, 0.0, False)] + \
    [("%s_%s" % (s, r), s, r, 1, 0.0, False) for s in ("S2", "S3", "S4", "S5") for r in REGIMES] + \
    [("S2_logits_d3", "S2", "logits", 3, 0.0, False),
     ("S1_logits_r3", "S1", "logits", 1, .3, False),
     ("S2_softmax_weighted", "S2", "softmax", 1, 0.0, True)]


def regime_inputs(regime, B, N, D=1, seed=SEED):
    """(B, N, D) f32 samples x, y of one input regime, from a seeded ``torch.Generator``:
    softmax  x = softmax(randn), y = softmax(3 randn): on the simplex, diameter ~ .35 (the suite's usual inputs)
    logits   x = randn, y = 1.5 randn: diameter ~ 8-10, where the loss depends on the schedule
    x30      30 * the softmax pair: diameter ~ 10, scaled intensities
    offset   the softmax pair + 10: |x| >> |x - y|, the expanded square of the cost"""
    g = torch.Generator().manual_seed(seed + 1000 * REGIMES.index(regime) + N + 7 * B + 131 * D)
    a, b = torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    if regime == "logits":
        return a, 1.5 * b
    x, y = torch.softmax(a, 1), torch.softmax(3 * b, 1)
    if regime == "x30":
        return 30 * x, 30 * y
    if regime == "offset":
        return x + 10, y + 10
    assert regime == "softmax", regime
    return x, y


def zero_mass_weights(B, N, seed=SEED):
    """Normalised (B, N) f32 weights with zero-mass anchors in both measures."""
    g = torch.Generator().manual_seed(seed + 1)
    a, b = torch.rand(B, N, generator=g), torch.rand(B, N, generator=g)
    a[:, ::7] = 0
    b[:, 3::11] = 0
    return a / a.sum(1, keepdim=True), b / b.sum(1, keepdim=True)


def run(crit, x, y, p, scaling, blur, reach, a=None, b=None):
    """loss, grad_x and the internals (schedule, diameter, final duals) of one reference call."""
    import geomloss.samples_loss as gsl
    x = x.clone().requires_grad_(True)
    cap = {}
    orig_sp, orig_cost = gsl.scaling_parameters, gsl.sinkhorn_cost

    def sp(*args, **k):
        r = orig_sp(*args, **k)
        cap["diameter"], cap["eps_s"], cap["rho"] = r[0], list(r[2]), r[3]
        return r

    def sc(eps, rho, al, be, a_x, b_y, a_y, b_x):
        cap["duals"] = np.stack([t.detach().numpy().copy() for t in (a_x, b_y, a_y, b_x)])
        return orig_cost(eps, rho, al, be, a_x, b_y, a_y, b_x)

    gsl.scaling_parameters, gsl.sinkhorn_cost = sp, sc
    try:
        if a is None:
            crit.p, crit.scaling, crit.blur, crit.reach = p, scaling, blur, (reach if reach > 0 else None)
            loss = crit(x, y)
        else:
            loss = crit.sinkhorn_tensorized(a, x, b, y, p=p, blur=blur, reach=reach if reach > 0 else None,
                                            diameter=None, scaling=scaling)
    finally:
        gsl.scaling_parameters, gsl.sinkhorn_cost = orig_sp, orig_cost
    loss.sum().backward()
    assert cap["rho"] == (reach ** p if reach > 0 else None)
    return {"loss": loss.detach().numpy(), "grad_x": x.grad.numpy(), "duals": cap["duals"],
            "eps_s": np.asarray(cap["eps_s"], dtype=np.float64), "diameter": np.float64(cap["diameter"])}


def gen_sinkhorn_regimes():
    import make_golden as mg  # the reference location and shims
    mg.install_shims()
    geomloss, gutils = mg.ref_geomloss()
    B, n = 2, 96
    out = {}
    for name, setting, regime, D, reach, weighted in REGIME_CASES:
        p, scaling, blur = SETTINGS[setting]
        x, y = regime_inputs(regime, B, n, D)
        crit = mg.ref_samples_loss(geomloss, gutils, n, B, blur)
        a = b = None
        if weighted:
            a, b = zero_mass_weights(B, n)
            out[name + "/alpha"], out[name + "/beta"] = a.numpy(), b.numpy()
        r = run(crit, x, y, p, scaling, blur, reach, a, b)
        out[name + "/x"], out[name + "/y"] = x.numpy(), y.numpy()
        for k, v in r.items():
            out[name + "/" + k] = v
        out[name + "/p"], out[name + "/scaling"] = np.int64(p), np.float64(scaling)
        out[name + "/blur"], out[name + "/reach"] = np.float64(blur), np.float64(reach)
        print("sinkhorn regimes", name, "n_eps", len(r["eps_s"]), "diameter %.5f" % r["diameter"],
              "loss", " ".join("%.6e" % v for v in r["loss"]))
    path = os.path.join(HERE, "sinkhorn_regimes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    gen_sinkhorn_regimes()
