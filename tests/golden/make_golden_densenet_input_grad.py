#!/usr/bin/env python
"""Generate tests/golden/densenet_input_grad.npz: the REFERENCE DenseNet's gradient with respect to its input image (CPU, f64).

Run only in the build container, where the reference checkout exists (see make_golden.py):

    python tests/golden/make_golden_densenet_input_grad.py

The reference's ``RegressionNetwork/DenseNet.py`` is imported as is, converted to f64 with ``.double()`` and loaded with
``oracle.deterministic_state_dict`` weights.  It runs in train mode (the mode the reference trains and tests in,
``train.py:42`` / ``test.py:36-37``).  The cotangent is a seeded standard-normal vector on each of the four heads, so the
stored gradient is the encoder's vector-Jacobian product with respect to ``x`` alone: ``d/dx sum_k <out[k], w[k]>``.

Two cases:
  * ``ref_b1_192x256``: B = 1 at the reference's native 192 x 256 crop and 96 anchors (its ``test.py`` batch size);
  * ``cfg2_b2_64x96``: B = 2 at 64 x 96 with ``fc`` / ``fc_dist`` swapped for matching ``nn.Linear`` (32 anchors), as
    ``make_golden.gen_densenet_cfg2`` does for the 240 x 320 geometry.

Stored per case: the seeds and shape of ``x`` (``x = default_rng(x_seed).random(shape, float32)``), the weight seed, the
four cotangents, the full f64 ``grad_x`` rounded to f32, and the relative L2 error of the reference's own f32 autograd
against that f64 gradient (the conditioning of the problem in f32).  The GPU tests read only the ``.npz``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference location and shims)

KEYS = ("distribution", "intensity", "rgb_ratio", "ambient")
CASES = [
    # name, B, crop, anchors, weight seed, x seed, cotangent seed
    ("ref_b1_192x256", 1, (192, 256), 96, 0, 60, 61),
    ("cfg2_b2_64x96", 2, (64, 96), 32, 3, 62, 63),
]


def _reference_net(crop, anchors, seed):
    sys.path.insert(0, os.path.join(mg.REF, "RegressionNetwork"))
    import DenseNet as refnet
    from oracle.densenet import deterministic_state_dict
    torch.manual_seed(0)
    net = refnet.DenseNet()
    if (crop, anchors) != ((192, 256), 96):   # the reference hard-codes fc for 192x256 and 96 anchors (DenseNet.py:125-126)
        h, w = crop[0] // 8 // 4, crop[1] // 8 // 4
        net.fc = torch.nn.Linear(171 * h * w, 1024)
        net.fc_dist = torch.nn.Linear(1024, anchors)
    net.load_state_dict(deterministic_state_dict(net.state_dict(), seed=seed))
    return net.train()


def _input_grad(net, x, w):
    x = x.clone().requires_grad_(True)
    out = net(x)
    sum((out[k] * w[k]).sum() for k in KEYS).backward()
    return x.grad.detach().double().numpy()


def gen_densenet_input_grad():
    out = {}
    for name, B, crop, anchors, wseed, xseed, gseed in CASES:
        x = mg.rng(xseed).random((B, 3) + crop, dtype=np.float32)
        g = mg.rng(gseed)
        w = {k: g.standard_normal((B, n)).astype(np.float32) for k, n in zip(KEYS, (anchors, 1, 3, 3))}
        net = _reference_net(crop, anchors, wseed)
        state = {k: v.clone() for k, v in net.state_dict().items()}
        g32 = _input_grad(net, torch.from_numpy(x), {k: torch.from_numpy(v) for k, v in w.items()})
        net.load_state_dict(state)   # the same running statistics for the f64 pass
        net = net.double()
        g64 = _input_grad(net, torch.from_numpy(x).double(), {k: torch.from_numpy(v).double() for k, v in w.items()})
        rel32 = float(np.linalg.norm(g32 - g64) / np.linalg.norm(g64))
        p = name + "/"
        out[p + "shape"] = np.array((B, 3) + crop, dtype=np.int64)
        out[p + "anchors"] = np.int64(anchors)
        out[p + "weight_seed"], out[p + "x_seed"] = np.int64(wseed), np.int64(xseed)
        for k in KEYS:
            out[p + "w_" + k] = w[k]
        out[p + "grad_x"] = g64.astype(np.float32)
        out[p + "ref_f32_rel_l2"] = np.float64(rel32)
        print("densenet input grad %s: |g| rms %.4g, reference f32 rel-L2 vs f64 %.3g" % (name, np.sqrt(np.mean(g64 ** 2)), rel32))
    np.savez_compressed(os.path.join(HERE, "densenet_input_grad.npz"), **out)


if __name__ == "__main__":
    mg.install_shims()
    gen_densenet_input_grad()
