#!/usr/bin/env python
"""Generate tests/golden/sinkhorn_dim.npz: the REFERENCE's Sinkhorn loss on D-dimensional samples, (B, N, D), on the CPU, f32.

Run only in the build container, where the reference checkout exists (see make_golden.py):

    python tests/golden/make_golden_sinkhorn_dim.py

The reference modules run unchanged (``ref_samples_loss`` builds the criterion for N anchors): ``spherical_distance``
takes any D (``utils.py:85-99``) and ``max_diameter`` the norm of the per-component ranges (``sinkhorn_divergence.py:9-18``).
Cases: D in {2, 3, 4}, the positional variant ``cat(dist, sphere_points)`` that ``spherical_distance`` carries commented
out, N in {96, 128, 256}, balanced and with a reach.  The weighted cases call ``sinkhorn_tensorized(alpha, x, beta, y, ...)``
directly -- the reference's own four-argument ``forward`` fails to unpack the six values ``process_args`` returns -- and
store the weights' gradients from its autograd.  Stored per case: x, y, (alpha, beta), loss, grad_x, (grad_alpha,
grad_beta), the final duals, eps_s, the diameter, blur and reach (0: balanced).  Arrays only; the GPU tests read only the
``.npz``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference location, shims and the Sinkhorn input recipes)

# name, kind, D, B, N, blur, reach (0: balanced), weighted
DIM_CASES = [
    ("d2_n96_softmax", "softmax", 2, 3, 96, .05, 0.0, False),
    ("d3_n128_rgb", "sparse", 3, 4, 128, .05, 0.0, False),          # per-anchor RGB distributions, cfg2's N
    ("d4_n128_positional", "positional", 4, 3, 128, .05, 0.0, False),   # cat(dist, sphere_points)
    ("d4_n96_positional_r1", "positional", 4, 2, 96, .025, .1, False),
    ("d2_n256_sparse", "sparse", 2, 2, 256, .05, 0.0, False),        # cfg5's N: the tiled kernel
    ("d3_n256_softmax_r3", "softmax", 3, 2, 256, .05, .3, False),
    ("d3_n96_weighted", "softmax", 3, 3, 96, .05, 0.0, True),
    ("d4_n256_positional_weighted_r1", "positional", 4, 2, 256, .05, .1, True),
]
SEED = 41


def dim_inputs(kind, D, B, n, seed):
    """(B, n, D) f32 samples: D independent draws of a 1-D recipe, or the distribution followed by the anchors' xyz."""
    if kind == "positional":
        x1, y1 = mg.sinkhorn_inputs("softmax", B, n, seed)
        a = torch.from_numpy(mg.ref_geomloss()[1].sphere_points(n)).float().numpy()
        pos = np.broadcast_to(a[None], (B, n, 3))
        return (np.concatenate([x1[:, :, None], pos], 2).astype(np.float32),
                np.concatenate([y1[:, :, None], pos], 2).astype(np.float32))
    xs, ys = zip(*[mg.sinkhorn_inputs(kind, B, n, seed + 97 * d) for d in range(D)])
    return np.stack(xs, 2).astype(np.float32), np.stack(ys, 2).astype(np.float32)


def weights(B, n, seed):
    g = np.random.default_rng(seed)
    a = g.random((B, n)).astype(np.float32)
    a[:, ::7] = 0
    b = g.random((B, n)).astype(np.float32)
    return (a / a.sum(1, keepdims=True)).astype(np.float32), (b / b.sum(1, keepdims=True)).astype(np.float32)


def run(crit, x_np, y_np, reach, a_np=None, b_np=None, blur=.05):
    """loss, the gradients and the internals (schedule, final duals) of one reference call."""
    import geomloss.samples_loss as gsl
    x = torch.from_numpy(x_np).requires_grad_(True)
    y = torch.from_numpy(y_np)
    cap = {}
    orig_sp, orig_cost = gsl.scaling_parameters, gsl.sinkhorn_cost

    def sp(*a, **k):
        r = orig_sp(*a, **k)
        cap["diameter"], cap["eps_s"], cap["rho"] = r[0], list(r[2]), r[3]
        return r

    def sc(eps, rho, a, b, a_x, b_y, a_y, b_x):
        cap["duals"] = np.stack([t.detach().numpy().copy() for t in (a_x, b_y, a_y, b_x)])
        return orig_cost(eps, rho, a, b, a_x, b_y, a_y, b_x)

    gsl.scaling_parameters, gsl.sinkhorn_cost = sp, sc
    try:
        if a_np is None:
            crit.reach = reach if reach > 0 else None
            loss = crit(x, y)
            a = b = None
        else:
            a = torch.from_numpy(a_np).requires_grad_(True)
            b = torch.from_numpy(b_np).requires_grad_(True)
            loss = crit.sinkhorn_tensorized(a, x, b, y, p=2, blur=blur, reach=reach if reach > 0 else None,
                                            diameter=None, scaling=.5)
    finally:
        gsl.scaling_parameters, gsl.sinkhorn_cost = orig_sp, orig_cost
    loss.sum().backward()
    out = {"loss": loss.detach().numpy(), "grad_x": x.grad.numpy(), "duals": cap["duals"],
           "eps_s": np.asarray(cap["eps_s"], dtype=np.float64), "diameter": np.float64(cap["diameter"])}
    if a is not None:
        out["grad_alpha"], out["grad_beta"] = a.grad.numpy(), b.grad.numpy()
    return out


def gen_sinkhorn_dim():
    geomloss, gutils = mg.ref_geomloss()
    out = {}
    for name, kind, D, B, n, blur, reach, weighted in DIM_CASES:
        x_np, y_np = dim_inputs(kind, D, B, n, SEED)
        assert x_np.shape == (B, n, D)
        crit = mg.ref_samples_loss(geomloss, gutils, n, B, blur)
        a_np = b_np = None
        if weighted:
            a_np, b_np = weights(B, n, SEED + 1)
            out[name + "/alpha"], out[name + "/beta"] = a_np, b_np
        r = run(crit, x_np, y_np, reach, a_np, b_np, blur)
        out[name + "/x"], out[name + "/y"] = x_np, y_np
        for k, v in r.items():
            out[name + "/" + k] = v
        out[name + "/blur"], out[name + "/reach"] = np.float64(blur), np.float64(reach)
        print("sinkhorn dim", name, "D", D, "n_eps", len(r["eps_s"]), "diameter %.5f" % r["diameter"],
              "loss0 %.4e" % r["loss"][0], "weighted" if weighted else "")
    np.savez_compressed(os.path.join(HERE, "sinkhorn_dim.npz"), **out)


if __name__ == "__main__":
    mg.install_shims()
    gen_sinkhorn_dim()
