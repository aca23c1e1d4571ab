"""``gmloss.SamplesLoss`` on the MI355X (reference ``RegressionNetwork/gmloss/samples_loss.py:12-84``).

``forward(x, y, geometry)``: ``geometry`` is the per-anchor depth; the reference rebuilds ``distance(batchsize,
geometry)`` on every call -- ``geometric_points`` (``gmloss/utils.py:63-74``) followed by an N^2 Python loop of
``torch.norm`` (``:76-92``, 16 384 tiny launches at N = 128) -- and then runs the same tensorised Sinkhorn as
``geomloss`` with cost ``(0.1 * |x_i - y_j|^2 + M_ij) / 2`` (``:94-108``, ``samples_loss.py:72-84``).

Here the ground cost is a *runtime argument* of the Sinkhorn kernel: the anchors are built in float64 on the host
(N numbers), ``eml_emd_anchor_cost_f32`` writes M on the device in one launch, and ``eml_sinkhorn_fwd_f32`` does the
rest -- the GMLight variant costs one extra 5 us launch per step.

A batch of crops from B scenes has B geometries (the reference's ``data.py:75`` loads a depth vector per sample, yet its
``distance(batchsize, geometry)`` repeats one matrix B times, ``gmloss/utils.py:89-93``): a ``(B, N)`` geometry goes to
``eml_gm_anchor_cost_f32`` -- anchors ``(B, N, 3)`` and chord matrices ``(B, N, N)`` in one launch, from a depth tensor that
stays on the device -- and the Sinkhorn kernels read sample b's matrix through a stride (``eml_sinkhorn_fwd_cost_f32``).
That path enqueues only: no host synchronisation.
"""
import numpy as np
import torch

from ... import _lib
from ..geomloss.samples_loss import SamplesLoss as _SphereSamplesLoss


def geometric_points(n=128, anchor_depth=None):
    """Depth-scaled Fibonacci anchors, float64 ``(n, 3)`` (``gmloss/utils.py:63-74``: radius = anchor_depth)."""
    golden_angle = np.pi * (3 - np.sqrt(5))
    theta = golden_angle * np.arange(n)
    z = np.linspace(1 - 1.0 / n, 1.0 / n - 1, n)
    radius = np.asarray(anchor_depth.detach().cpu().numpy() if isinstance(anchor_depth, torch.Tensor) else anchor_depth,
                        dtype=np.float64)
    points = np.zeros((n, 3))
    points[:, 0] = radius * np.cos(theta)
    points[:, 1] = radius * np.sin(theta)
    points[:, 2] = z
    return points


class SamplesLoss(_SphereSamplesLoss):
    """``SamplesLoss(loss="sinkhorn", p=2, blur=.05, reach=None, diameter=None, scaling=.5, batchsize=None)``,
    ``forward(x, y, geometry) -> (B,)`` with x, y of shape (B, 128, 1).  ``anchors`` lifts the reference's hard-coded
    N = 128 (``gmloss/utils.py:78``).  ``reach`` (unbalanced OT, the fork's damped loop and loss) works as in
    ``geomloss.SamplesLoss``: ``forward`` runs the parent's, which passes ``reach**p`` to the kernel."""

    def __init__(self, loss="sinkhorn", p=2, blur=.05, reach=None, diameter=None, scaling=.5, batchsize=None,
                 anchors=128):
        super().__init__(loss, p, blur, reach, diameter, scaling, batchsize, anchors=anchors)

    def _forward_per_sample(self, x, y, depth):
        """``geometry`` of shape ``(B, N)``: one depth vector per sample."""
        B = x.shape[0]
        if tuple(depth.shape) != (B, self.N):
            raise ValueError("a per-sample geometry must be (B, N) = (%d, %d) like x %s, got %s"
                             % (B, self.N, tuple(x.shape), tuple(depth.shape)))
        depth = depth.detach()
        if depth.dtype not in (torch.float32, torch.float64):
            depth = depth.float()
        depth = _lib.require_gpu_tensor(depth.to(x.device), "geometry", depth.dtype)   # a CPU tensor: the one copy
        a = torch.empty(B, self.N, 3, dtype=torch.float32, device=depth.device)
        M = torch.empty(B, self.N, self.N, dtype=torch.float32, device=depth.device)
        if B > 0:
            _lib.check(_lib.lib().eml_gm_anchor_cost_f32(_lib.ptr(depth), int(depth.dtype == torch.float64), B, self.N,
                                                         _lib.ptr(a), _lib.ptr(M), _lib.current_stream()),
                       "eml_gm_anchor_cost_f32")
        self.anchors = a
        self.M, self.Mt = M, M  # every sample's matrix is symmetric: the transposes alias
        return super().forward(x, y)

    def forward(self, x, y, geometry):
        """``geometry``: the per-anchor depth, ``(N,)`` (tensor, array or list) for the whole batch as in the reference, or
        ``(B, N)`` (f32 or f64 tensor, on the device or not; an array or nested list works too) with one row per sample.
        ``self.anchors`` / ``self.M`` hold the call's anchors and chord matrices: ``(N, 3)`` / ``(N, N)``, or ``(B, N, 3)`` /
        ``(B, N, N)``."""
        if not isinstance(geometry, torch.Tensor) and np.ndim(geometry) == 2:
            geometry = torch.as_tensor(np.asarray(geometry))
        if isinstance(geometry, torch.Tensor) and geometry.dim() == 2:
            return self._forward_per_sample(x, y, geometry)
        dev = x.device
        a = torch.from_numpy(geometric_points(self.N, geometry)).float().to(dev).contiguous()
        if not a.is_cuda:
            raise _lib.EmlightHipError("gmloss.SamplesLoss needs tensors on the MI355X; there is no CPU path")
        M = torch.empty(self.N, self.N, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().eml_emd_anchor_cost_f32(_lib.ptr(a), _lib.ptr(M), self.N, _lib.current_stream()),
                   "eml_emd_anchor_cost_f32")
        self.anchors = a
        self.M, self.Mt = M, M  # symmetric: the transpose aliases
        return super().forward(x, y)
