#!/usr/bin/env python
"""Generate tests/golden/gmloss_batched.npz: the REAL reference's ``gmloss.SamplesLoss`` run once per sample, each sample
with its own depth vector -- what a batch of crops from B scenes should compute (the reference itself repeats one
geometry ``batchsize`` times, ``gmloss/utils.py:89-93``).

Run only where the reference tree exists (see ``make_golden.py``):

    python tests/golden/make_golden_gmloss_batched.py

The regime is one where the chord matrix matters (at EMLight's operating point, blur .05 and values ~ 1/N, the transport
plan is the identity and the loss does not depend on M at all): blur .5, samples 30 * softmax, depths U(.05, 3) drawn
independently per sample, one diameter for the whole batch.  ``batched_inputs`` is imported by the GPU tests."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import make_golden as mg  # noqa: E402

SEED, B, N, BLUR = 23, 3, 128, .5


def batched_inputs(B, n, seed=SEED, D=1):
    """x, y ``(B, n)`` (``(B, n, D)`` for D > 1) f32 = 30 * ``make_golden.sinkhorn_inputs("softmax", ...)`` and depth
    ``(B, n)`` f64, U(.05, 3), every sample's row drawn on its own."""
    xs, ys = zip(*(mg.sinkhorn_inputs("softmax", B, n, seed + d) for d in range(D)))
    x = np.float32(30.0) * (xs[0] if D == 1 else np.stack(xs, -1))
    y = np.float32(30.0) * (ys[0] if D == 1 else np.stack(ys, -1))
    depth = np.stack([mg.rng(seed, n, b).uniform(0.05, 3.0, n) for b in range(B)])
    return x, y, depth


def batch_diameter(x, y):
    """``max_diameter`` (sinkhorn_divergence.py:9-18) of the whole batch, as a Python float."""
    D = 1 if x.ndim == 2 else x.shape[-1]
    xf, yf = torch.from_numpy(x).reshape(-1, D), torch.from_numpy(y).reshape(-1, D)
    mins = torch.minimum(xf.min(0)[0], yf.min(0)[0])
    maxs = torch.maximum(xf.max(0)[0], yf.max(0)[0])
    return (maxs - mins).norm().item()


def main():
    mg.install_shims()
    sys.path.insert(0, os.path.join(mg.REF, "RegressionNetwork"))
    import gmloss  # noqa: the reference package
    x_np, y_np, depth = batched_inputs(B, N)
    diameter = batch_diameter(x_np, y_np)
    out = {"blur": np.float64(BLUR), "diameter": np.float64(diameter), "loss": [], "grad_x": [], "M_rows8": [], "anchors": []}
    for b in range(B):
        x = torch.from_numpy(x_np[b:b + 1]).view(1, N, 1).requires_grad_(True)
        y = torch.from_numpy(y_np[b:b + 1]).view(1, N, 1)
        crit = gmloss.SamplesLoss("sinkhorn", p=2, blur=BLUR, diameter=diameter, batchsize=1)
        loss = crit(x, y, depth[b])
        loss.sum().backward()
        out["loss"].append(loss.detach().numpy()[0])
        out["grad_x"].append(x.grad.numpy().reshape(N))
        out["M_rows8"].append(crit.distance.M[0, ::8].numpy())
        out["anchors"].append(crit.distance.anchors[0].numpy())
        print("gmloss_batched sample", b, "loss %.6e" % float(loss[0]))
    np.savez_compressed(os.path.join(HERE, "gmloss_batched.npz"), **{k: np.asarray(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
