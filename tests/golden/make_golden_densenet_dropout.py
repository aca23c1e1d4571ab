#!/usr/bin/env python
"""Generate tests/golden/densenet_dropout.npz: the REFERENCE DenseNet with ``drop_rate=0.2`` (CPU, f64), its dropout masks
taken from the hash the HIP kernels use (tests/dropout_hash.py) for a fixed key.

Run only in the build container, where the reference checkout exists (see make_golden.py):

    python tests/golden/make_golden_densenet_dropout.py

The reference's ``RegressionNetwork/DenseNet.py`` is imported as is, with ``drop_rate=0.2`` and the weights of
``oracle.deterministic_state_dict``.  The ``F.dropout`` its ``_DenseLayer.forward`` calls (DenseNet.py:50-55) is replaced by a
shim that multiplies in the masks of the numpy restatement of the kernels' hash, layer after layer in call order (global dense
layer index 0..47).  Train mode, B = 2 at the reference's native 192 x 256 (its ``fc`` is hard-wired to 8208 = 171 x 6 x 8),
96 anchors.  The cotangent is a seeded standard-normal vector on each head.

Stored: the shape and seeds of ``x`` (``x = default_rng(x_seed).random(shape, float32)``), the weight seed, the key, p, the
four f64 outputs, ``grad_x`` of image 0 (image 1's would take the file over 1 MB), the gradients of a sample of parameters,
the per-tensor L2 norms of every parameter gradient, and for each stored gradient the relative L2 error of the reference's own
f32 autograd (same masks) against f64.  The GPU tests read only the ``.npz``.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402  (the reference location and shims)
from tests.dropout_hash import scaled_mask_nchw  # noqa: E402

KEYS = ("distribution", "intensity", "rgb_ratio", "ambient")
B, CROP, ANCHORS, P_DROP = 2, (192, 256), 96, 0.2
WSEED, XSEED, GSEED = 5, 70, 71
KEY = 0x9E3779B97F4A7C15
SAMPLE = ["features.conv0.weight", "features.norm0.weight",
          "features.denseblock1.denselayer1.conv2.weight", "features.denseblock1.denselayer16.conv2.weight",
          "features.denseblock1.denselayer16.norm2.weight", "features.denseblock2.denselayer8.conv2.weight",
          "features.denseblock2.denselayer8.conv1.weight", "features.denseblock3.denselayer16.conv2.weight",
          "features.denseblock3.denselayer1.norm1.weight", "features.transition1.conv.weight",
          "features.last_norm3.bias", "fc_intensity.weight"]


class _MaskedDropout:
    """F.dropout of the reference module: the hash's masks, one layer per call in call order."""

    def __init__(self, key):
        self.key, self.layer = key, 0

    def __call__(self, t, p=0.5, training=True, inplace=False):
        assert training and p == P_DROP
        b, c, h, w = t.shape
        m = torch.from_numpy(scaled_mask_nchw(self.key, self.layer, p, b, h, w)).to(t.dtype)
        self.layer += 1
        return t * m


def _reference_net():
    sys.path.insert(0, os.path.join(mg.REF, "RegressionNetwork"))
    import DenseNet as refnet
    from oracle.densenet import deterministic_state_dict
    torch.manual_seed(0)
    net = refnet.DenseNet(drop_rate=P_DROP)
    net.load_state_dict(deterministic_state_dict(net.state_dict(), seed=WSEED))
    return refnet, net.train()


def _run(refnet, net, x, w):
    shim = _MaskedDropout(KEY)
    refnet.F = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("_")})
    refnet.F.dropout = shim
    x = x.clone().requires_grad_(True)
    net.zero_grad(set_to_none=True)
    out = net(x)
    assert shim.layer == 48
    sum((out[k] * w[k]).sum() for k in KEYS).backward()
    grads = {n: q.grad.detach().double().numpy() for n, q in net.named_parameters()}
    return ({k: v.detach().double().numpy() for k, v in out.items()}, x.grad.detach().double().numpy(), grads)


def gen_densenet_dropout():
    x = mg.rng(XSEED).random((B, 3) + CROP, dtype=np.float32)
    g = mg.rng(GSEED)
    w = {k: g.standard_normal((B, n)).astype(np.float32) for k, n in zip(KEYS, (ANCHORS, 1, 3, 3))}
    refnet, net = _reference_net()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    _, gx32, gp32 = _run(refnet, net, torch.from_numpy(x), {k: torch.from_numpy(v) for k, v in w.items()})
    net.load_state_dict(state)   # the same running statistics for the f64 pass
    net = net.double()
    out64, gx64, gp64 = _run(refnet, net, torch.from_numpy(x).double(), {k: torch.from_numpy(v).double() for k, v in w.items()})
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    out = {"shape": np.array((B, 3) + CROP, dtype=np.int64), "anchors": np.int64(ANCHORS), "weight_seed": np.int64(WSEED),
           "x_seed": np.int64(XSEED), "key": np.uint64(KEY), "p": np.float64(P_DROP)}
    for k in KEYS:
        out["w_" + k] = w[k]
        out["out_" + k] = out64[k]
    out["grad_x0"] = gx64[0].astype(np.float32)
    out["grad_x0_ref_f32_rel_l2"] = np.float64(rel(gx32[0], gx64[0]))
    for n in SAMPLE:
        out["grad/" + n] = gp64[n].astype(np.float32)
        out["ref_f32_rel_l2/" + n] = np.float64(rel(gp32[n], gp64[n]))
    names = [n for n, _ in net.named_parameters()]
    out["param_names"] = np.array(names)
    out["param_grad_l2"] = np.array([np.linalg.norm(gp64[n]) for n in names])
    np.savez_compressed(os.path.join(HERE, "densenet_dropout.npz"), **out)
    print("densenet dropout: dX rel f32 %.3g; sample %s" % (out["grad_x0_ref_f32_rel_l2"],
          ", ".join("%.2g" % out["ref_f32_rel_l2/" + n] for n in SAMPLE)))


if __name__ == "__main__":
    mg.install_shims()
    gen_densenet_dropout()
