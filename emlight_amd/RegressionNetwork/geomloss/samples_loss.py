"""``SamplesLoss`` -- EMLight's spherical mover's (Sinkhorn) loss on the MI355X.

Same constructor and ``forward`` as the reference class
(``RegressionNetwork/geomloss/samples_loss.py:12-92``); the body is one call into
``libemlight_hip.so`` (``eml_sinkhorn_schedule_f32`` + ``eml_sinkhorn_fwd_f32``) instead of
four materialised (B,N,N) cost tensors and ~250 ATen launches.  Extra, optional arguments
lift what the reference hard-codes: ``anchors`` (reference: 96, ``geomloss/utils.py:66``)
and ``cost_matrix`` (a runtime (N,N) ground cost -- gives the GMLight variant,
``gmloss/utils.py:63-108``, for free).  ``batchsize`` is accepted and ignored: the chord
matrix is stored once, not ``batchsize`` times (``utils.py:80-81``).

``reach`` (unbalanced OT) follows EMLight's fork: ``rho = reach**p`` (``sinkhorn_divergence.py:35``) damps every softmin of
the loop by ``1 / (1 + eps / rho)`` (``:43-44, 78-107``; ``eml_sinkhorn_fwd_rho_f32``), and the loss is the fork's
``<alpha, b_x - a_x> + <beta, a_y - b_y>`` of the damped duals (``:65-69``, which ignores rho) -- not upstream geomloss's
unbalanced divergence with its exponentially transformed dual terms.

Samples may be D-dimensional, ``(B, N, D)`` with ``1 <= D <= MAX_DIM`` as in the reference (``utils.py:85-99``: the cost
``.5 * (.1 * |x_i - y_j|^2 + M_ij)``; ``sinkhorn_divergence.py:9-18``: the diameter over the per-component ranges);
``D = 1`` makes exactly the calls it always made, ``D > 1`` calls ``eml_sinkhorn_fwd_dim_f32``.  Weights passed in the
four- or six-argument form get gradients when they require them: ``(b_x - a_x)`` and ``(a_y - b_y)`` of the final duals
(``:65-69``; the weights enter the loop only through detached log-weights), ``eml_sinkhorn_bwd_weights_f32``.

The ground cost may differ per sample: a ``(B, N, N)`` matrix (``forward(..., cost_matrix=)``, or what
``gmloss.SamplesLoss`` builds from per-sample depths) goes to ``eml_sinkhorn_fwd_cost_f32`` with a stride of ``N*N`` floats;
an ``(N, N)`` matrix makes exactly the calls it always made.
"""
import math

import torch
from torch.nn import Module

from ... import _lib
from ..util import sphere_points


EML_SINKHORN_NO_SPLIT, EML_SINKHORN_FORCE_SPLIT, EML_SINKHORN_TEST_STALL = 1, 2, 4   # include/emlight_hip.h
MAX_DIM = 8   # EML_SINKHORN_MAX_DIM: the largest point dimension D the kernels take


def split_eligible(N):
    """Shapes whose small batches may take the split kernel (csrc/sinkhorn.hip; the only path that has a status word)."""
    return 192 <= N <= 512 and N % 64 == 0


class _SplitWatch:
    """Host side of the split kernel's fail-safe.  The library already made the result right on the device (the tiled
    kernel recomputes a batch whose split kernel gave up: slices not co-resident -- a CU-masked or shared GPU, another
    stream's kernel); what is left for the host is to NOTICE, so that the next calls stop paying the 50 ms give-up: the
    status word of a call is copied to pinned memory without a sync (first three calls, then every 64th) and read when a
    later call finds the copy complete -- the pattern of the dense engine's dgamma ring.  Once raised, this process passes
    EML_SINKHORN_NO_SPLIT from then on."""

    def __init__(self):
        self.disabled = False
        self.fallbacks = 0
        self.calls = 0
        self.pending = None   # (pinned int32 tensor, event)

    def flags(self):
        self.poll()
        return EML_SINKHORN_NO_SPLIT if self.disabled else 0

    def poll(self, wait=False):
        if self.pending is None:
            return
        host, ev = self.pending
        if wait:
            ev.synchronize()
        elif not ev.query():
            return
        self.pending = None
        if int(host[0]) != 0:
            self.fallbacks += 1
            if not self.disabled:
                import warnings
                warnings.warn("emlight_amd: the split Sinkhorn kernel's workgroups were not co-resident (CU mask, shared "
                              "GPU or a concurrent kernel); the tiled kernel recomputed the batch. The split path is "
                              "disabled for the rest of this process.", RuntimeWarning, stacklevel=3)
            self.disabled = True

    def after_call(self, work, B, N):
        self.calls += 1
        if self.disabled or self.pending is not None or not (self.calls <= 3 or self.calls % 64 == 0):
            return
        host = torch.empty(1, dtype=torch.int32).pin_memory()
        with torch.cuda.device(work.device):   # copy and event on the device (and its current stream) that ran the call
            host.copy_(work[24 * B * N:24 * B * N + 1].view(torch.int32), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.pending = (host, ev)


_split_watches = {}


def split_watch(device):
    """The watch of one device: whether the slices of the split kernel are co-resident is a property of the device (and of
    what shares it), so a give-up on one GPU must not disable the path on the others of a process."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _split_watches:
        _split_watches[idx] = _SplitWatch()
    return _split_watches[idx]


MAX_EPS = 64   # EML_MAX_EPS: the entries of the caller-owned schedule buffers, and one entry per lane in the kernels


def schedule_length(p, diameter, blur, scaling):
    """Entries of the epsilon schedule ``[d^p] + [exp(e) for e in arange(p ln d, p ln blur, p ln scaling)] + [blur^p]``
    (``sinkhorn_divergence.py:21-25``) of a diameter ``d > 0``: 2 + the ``numpy.arange`` length, by the kernels' own f64
    formula (csrc/sinkhorn.hip, ``device_schedule``).  A schedule of more than ``MAX_EPS`` entries is refused, not cut."""
    if not diameter > 0:
        raise ValueError("the diameter must be > 0, got %r" % (diameter,))
    cnt = math.ceil((p * math.log(blur) - p * math.log(diameter)) / (p * math.log(scaling)))
    return 2 + max(0, cnt)


def reach_to_rho(reach, p):
    """``rho = reach**p`` (sinkhorn_divergence.py:35) for a validated ``reach``, or None (balanced) for ``reach=None``.
    ``reach`` must be a number > 0; ``float('inf')`` is accepted and gives lam = 1 (the balanced numbers)."""
    if reach is None:
        return None
    try:
        r = float(reach)
    except (TypeError, ValueError):
        raise ValueError("reach must be None or a number > 0, got %r" % (reach,)) from None
    if not r > 0:   # also NaN
        raise ValueError("reach must be None or a number > 0, got %r" % (reach,))
    try:
        return r ** p
    except OverflowError:
        return math.inf


def sinkhorn_outputs(B, N, dev, need_gx=True, need_gy=False, D=1):
    """Device buffers one forward call writes (the caller owns every buffer, include/emlight_hip.h): those of
    ``eml_sinkhorn_fwd_ex_f32`` / ``_rho_f32`` for ``D = 1``, those of ``eml_sinkhorn_fwd_dim_f32`` -- gradients
    ``(B, N, D)``, its own scratch size -- for ``D > 1``."""
    f32 = dict(dtype=torch.float32, device=dev)
    # scratch size from the library (duals, expectation rows; D = 1: the small-batch kernel's exchange buffer and status
    # words too); never less than the planes every kernel writes
    if D == 1:
        n_work = max(int(_lib.lib().eml_sinkhorn_work_floats(B, N)), 8 * B * N)
    else:
        n_work = max(int(_lib.lib().eml_sinkhorn_dim_work_floats(B, N, D)), (4 + 4 * D) * B * N)
    work = torch.empty(n_work, **f32)
    if D == 1 and split_eligible(N) and n_work > 24 * B * N:
        work[24 * B * N:].zero_()   # the status word: only calls that take the split path reset it
    grad = (B, N) if D == 1 else (B, N, D)
    return {"eps_s": torch.empty(64, **f32), "n_eps": torch.empty(1, dtype=torch.int32, device=dev),
            "diameter": torch.empty(1, **f32), "loss": torch.empty(B, **f32),
            "gx": torch.empty(grad, **f32) if need_gx else None, "gy": torch.empty(grad, **f32) if need_gy else None,
            "work": work}


def global_range(x, y):
    """(2,) tensor (min, max) of x U y over the batch of EVERY data-parallel rank, without a host sync: the local extrema,
    then ONE 2-float all-reduce (MIN over (min, -max)).  ``max_diameter`` (sinkhorn_divergence.py:9-18) takes the range
    over the whole batch, so a rank that only scanned its own shard would derive a different eps-schedule than the
    single-process run with the global batch.  With one rank this is just the local range.
    ``x, y`` of shape ``(B, N, D)``: the (2*D,) per-component minima then maxima (``max_diameter`` takes the norm of the
    per-component ranges), all-reduced in the same one call."""
    import torch.distributed as dist
    from ..._dist import dp_active
    if x.dim() == 3:
        D = x.shape[-1]
        lo = torch.minimum(x.detach().reshape(-1, D).amin(0), y.detach().reshape(-1, D).amin(0))
        hi = torch.maximum(x.detach().reshape(-1, D).amax(0), y.detach().reshape(-1, D).amax(0))
        r = torch.cat([lo, -hi]).float()
        if dp_active():
            dist.all_reduce(r, op=dist.ReduceOp.MIN)
        return torch.cat([r[:D], -r[D:]])
    lo = torch.minimum(x.detach().amin(), y.detach().amin())
    hi = torch.maximum(x.detach().amax(), y.detach().amax())
    r = torch.stack([lo, -hi]).float()
    if dp_active():
        dist.all_reduce(r, op=dist.ReduceOp.MIN)
    return torch.stack([r[0], -r[1]])


def sinkhorn_raw(x, y, alpha, beta, M, Mt, p, blur, scaling, diameter, need_gx=True, need_gy=False, out=None,
                 range_lo_hi=None, flags=None, rho=None, want_lam=False):
    """One call into the HIP library; returns every device-side output (no autograd).  ``out``: buffers from
    ``sinkhorn_outputs`` to write into (a timing loop passes them so that no allocation sits between launches).
    ``range_lo_hi``: device tensor from ``global_range`` -- the kernel folds it into its own scan.
    ``x, y`` of shape ``(B, N)`` (1-D points) or ``(B, N, D)`` (``eml_sinkhorn_fwd_dim_f32``; the split kernel and its
    watch do not apply there).
    ``flags``: EML_SINKHORN_* of the C ABI; default: whatever the split kernel's watch says (``_SplitWatch``).
    ``rho``: reach**p of unbalanced OT, or None (balanced; for 1-D points the call is ``eml_sinkhorn_fwd_ex_f32``, as
    it always was); ``want_lam``: also return the dampening schedule ``lam`` (64 floats next to ``eps_s``; all ones when
    balanced).
    ``M, Mt``: ``(N, N)``, one ground cost for the batch, or ``(B, N, N)``, one per sample (``eml_sinkhorn_fwd_cost_f32``
    with stride ``N*N``; the split kernel and its watch apply as with one matrix)."""
    L = _lib.lib()
    B, N = x.shape[:2]
    per_sample = M.dim() == 3
    if per_sample and (tuple(M.shape) != (B, N, N) or tuple(Mt.shape) != (B, N, N)):
        raise ValueError("a per-sample ground cost must be (B, N, N) = (%d, %d, %d), got M %s and Mt %s"
                         % (B, N, N, tuple(M.shape), tuple(Mt.shape)))
    D = x.shape[2] if x.dim() == 3 else None   # None: 1-D points through the entries that take no D
    o = out if out is not None else sinkhorn_outputs(B, N, x.device, need_gx, need_gy, D=D or 1)
    watched = D is None and flags is None and split_eligible(N)
    if watched:
        flags = split_watch(x.device).flags()
    lam = None
    if want_lam:
        lam = o.get("lam")
        lam = torch.empty(64, dtype=torch.float32, device=x.device) if lam is None else lam
    args = (_lib.ptr(x), _lib.ptr(y), _lib.ptr(M), _lib.ptr(Mt), _lib.ptr(alpha), _lib.ptr(beta),
            float(blur), float(scaling), int(p), float(diameter) if diameter is not None else -1.0,
            _lib.ptr(range_lo_hi), _lib.ptr(o["eps_s"]), _lib.ptr(o["n_eps"]), _lib.ptr(o["diameter"]), _lib.ptr(o["loss"]),
            _lib.ptr(o["gx"]), _lib.ptr(o["gy"]), _lib.ptr(o["work"]), B, N)
    flags, stream = int(flags or 0), _lib.current_stream()
    rho_lam = (float(rho) if rho is not None else 0.0, _lib.ptr(lam))
    if per_sample:
        _lib.check(L.eml_sinkhorn_fwd_cost_f32(*args, D or 1, flags, *rho_lam, N * N, stream), "eml_sinkhorn_fwd_cost_f32")
    elif D is not None:
        _lib.check(L.eml_sinkhorn_fwd_dim_f32(*args, D, flags, *rho_lam, stream), "eml_sinkhorn_fwd_dim_f32")
    elif rho is None and not want_lam:
        _lib.check(L.eml_sinkhorn_fwd_ex_f32(*args, flags, stream), "eml_sinkhorn_fwd_ex_f32")
    else:
        _lib.check(L.eml_sinkhorn_fwd_rho_f32(*args, flags, *rho_lam, stream), "eml_sinkhorn_fwd_rho_f32")
    if watched and o["work"].numel() > 24 * B * N:
        split_watch(x.device).after_call(o["work"], B, N)
    r = {"loss": o["loss"], "gx": o["gx"], "gy": o["gy"], "eps_s": o["eps_s"], "n_eps": o["n_eps"],
         "diameter": o["diameter"], "duals": o["work"][:4 * B * N].view(4, B, N), "work": o["work"]}
    if lam is not None:
        r["lam"] = lam
    return r


class _SinkhornDivergence(torch.autograd.Function):
    """loss (B,) = S_eps(alpha@x, beta@y).  Backward = analytic gradient of the last
    extrapolation (``sinkhorn_divergence.py:101-107``), produced by the forward kernel.  ``rho``: reach**p or None.
    ``x, y``: (B, N) or (B, N, D).  Weights that require grad get ``gloss * (b_x - a_x)`` / ``gloss * (a_y - b_y)`` from the
    final duals the forward left in its scratch (``eml_sinkhorn_bwd_weights_f32``)."""

    @staticmethod
    def forward(ctx, x, y, alpha, beta, M, Mt, p, blur, scaling, diameter, range_lo_hi=None, rho=None):
        r = sinkhorn_raw(x, y, alpha, beta, M, Mt, p, blur, scaling, diameter,
                         ctx.needs_input_grad[0], ctx.needs_input_grad[1], range_lo_hi=range_lo_hi, rho=rho)
        ctx.want_weights = (alpha is not None and ctx.needs_input_grad[2], beta is not None and ctx.needs_input_grad[3])
        ctx.BN = (x.shape[0], x.shape[1])
        ctx.save_for_backward(r["gx"], r["gy"], r["work"] if any(ctx.want_weights) else None)
        return r["loss"]

    @staticmethod
    def backward(ctx, gloss):
        gx_u, gy_u, work = ctx.saved_tensors
        L = _lib.lib()
        gloss = gloss.contiguous()
        out = [None, None, None, None]
        for k, gu in enumerate((gx_u, gy_u)):
            if gu is None:
                continue
            B, N = gu.shape[0], gu[0].numel()   # (B, N) or (B, N, D): the same row scaling
            go = torch.empty_like(gu)
            _lib.check(L.eml_sinkhorn_bwd_f32(_lib.ptr(gloss), _lib.ptr(gu), _lib.ptr(go), B, N,
                                              _lib.current_stream()), "eml_sinkhorn_bwd_f32")
            out[k] = go
        if work is not None:
            B, N = ctx.BN
            ga = torch.empty(B, N, dtype=torch.float32, device=gloss.device) if ctx.want_weights[0] else None
            gb = torch.empty(B, N, dtype=torch.float32, device=gloss.device) if ctx.want_weights[1] else None
            _lib.check(L.eml_sinkhorn_bwd_weights_f32(_lib.ptr(gloss), _lib.ptr(work), _lib.ptr(ga), _lib.ptr(gb), B, N,
                                                      _lib.current_stream()), "eml_sinkhorn_bwd_weights_f32")
            out[2], out[3] = ga, gb
        return out[0], out[1], out[2], out[3], None, None, None, None, None, None, None, None


class SamplesLoss(Module):
    """Debiased Sinkhorn divergence between sampled measures on the N sphere anchors.

    ``SamplesLoss(loss="sinkhorn", p=2, blur=.05, reach=None, diameter=None, scaling=.5,
    batchsize=None)`` -- reference signature ``samples_loss.py:22``; ``forward(x, y)`` with
    ``x, y`` of shape ``(B, N, D)``, ``1 <= D <= 8``, returns ``(B,)`` (``samples_loss.py:35-46``); the gradients have
    the shape of ``x``, ``y``.  In the four- and six-argument forms, weights that require grad get gradients too.

    ``reach``: None (balanced OT) or a number > 0 (``float('inf')`` included; anything else raises ``ValueError``).
    With a reach, every softmin of the Sinkhorn loop is damped by ``1 / (1 + eps / reach**p)`` as in EMLight's fork
    (``sinkhorn_divergence.py:35, 43-44, 78-107``); the loss stays the fork's ``<alpha, b_x - a_x> + <beta, a_y - b_y>``
    of the damped duals (``:65-69``), NOT upstream geomloss's unbalanced divergence.

    The epsilon schedule (``schedule_length``) holds at most ``MAX_EPS`` = 64 entries (p = 2, diameter 1, blur .05:
    ``scaling <= .95``).  A longer one is refused, never cut short: with a fixed ``diameter`` the constructor raises
    ``ValueError``; with the diameter taken from the data the call returns NaN losses and gradients, and ``forward_raw``
    reports ``n_eps = -(entries needed)``.  Samples whose diameter is not > 0 (x and y constant and equal; the reference
    raises there) give NaN too, with ``n_eps = 0``.
    """

    def __init__(self, loss="sinkhorn", p=2, blur=.05, reach=None, diameter=None, scaling=.5,
                 batchsize=None, anchors=96, cost_matrix=None, sync_diameter=False):
        super().__init__()
        if loss != "sinkhorn":
            raise ValueError("only loss='sinkhorn' exists in EMLight's geomloss fork")
        self.rho = reach_to_rho(reach, p)   # validates reach
        self.loss, self.p, self.blur, self.reach = loss, p, blur, reach
        self.diameter, self.scaling = diameter, scaling
        if diameter is not None and diameter > 0 and blur > 0 and 0 < scaling < 1 and p >= 1:
            need = schedule_length(p, diameter, blur, scaling)
            if need > MAX_EPS:
                raise ValueError("the epsilon schedule of p=%r, diameter=%r, blur=%r, scaling=%r has %d entries; the HIP "
                                 "kernels hold at most %d (EML_MAX_EPS): raise blur or lower scaling"
                                 % (p, diameter, blur, scaling, need, MAX_EPS))
        # data-parallel training: derive the eps-schedule from the range of the GLOBAL batch (one 2-float all-reduce per
        # call, no host sync) -- what the single-process reference sees; ignored when ``diameter`` is given
        self.sync_diameter = bool(sync_diameter)
        self.N = int(anchors) if cost_matrix is None else int(cost_matrix.shape[-1])
        # anchors as the reference builds them: float64 Fibonacci sphere cast to f32 (utils.py:67-69)
        self.register_buffer("anchors", torch.from_numpy(sphere_points(self.N)).float(), persistent=False)
        if cost_matrix is not None:
            M = torch.as_tensor(cost_matrix, dtype=torch.float32).reshape(self.N, self.N).clone()
            self.register_buffer("M", M, persistent=False)
            self.register_buffer("Mt", M.t().contiguous(), persistent=False)
        else:
            self.M = None
            self.Mt = None

    def cost_matrix(self, device):
        """(N,N) chord matrix on ``device`` -- built once by ``eml_emd_anchor_cost_f32``."""
        if self.M is None or self.M.device != device:
            if self.M is not None:  # user-supplied matrix: just move it
                self.M, self.Mt = self.M.to(device), self.Mt.to(device)
            else:
                a = self.anchors.to(device).contiguous()
                M = torch.empty(self.N, self.N, dtype=torch.float32, device=device)
                _lib.check(_lib.lib().eml_emd_anchor_cost_f32(_lib.ptr(a), _lib.ptr(M), self.N,
                                                              _lib.current_stream()), "eml_emd_anchor_cost_f32")
                self.M, self.Mt = M, M  # symmetric: the transpose aliases
        return self.M, self.Mt

    @staticmethod
    def generate_weights(x):
        if x.dim() == 3:
            B, N, _ = x.shape
            return torch.ones(B, N).type_as(x) / N
        raise ValueError("Input samples 'x' and 'y' should be encoded as (B,N,D) (batch) tensors.")

    def process_args(self, *args):
        if len(args) == 6:
            _, a, x, _, b, y = args
            return a, x, b, y
        if len(args) == 4:
            return args
        if len(args) == 2:
            x, y = args
            return None, x, None, y  # uniform 1/N weights are generated inside the kernel
        raise ValueError("A SamplesLoss accepts two (x, y), four (a, x, b, y) or six (l_x, a, x, l_y, b, y) arguments.")

    def _check_samples(self, x, y):
        """The point dimension D of ``x, y`` (both ``(B, N, D)``, 1 <= D <= MAX_DIM), or ValueError."""
        if x.dim() != 3 or y.shape != x.shape or x.shape[1] != self.N:
            raise ValueError("expected x, y of the same shape (B, %d, D), got %s and %s"
                             % (self.N, tuple(x.shape), tuple(y.shape)))
        D = x.shape[-1]
        if not 1 <= D <= MAX_DIM:
            raise ValueError("the point dimension D must be 1 <= D <= %d (EML_SINKHORN_MAX_DIM), got D = %d" % (MAX_DIM, D))
        return D

    def _samples(self, x, y):
        """``x, y`` as the kernels read them: ``(B, N)`` for 1-D points, ``(B, N, D)`` for D > 1."""
        if not (x.dim() == 3 and x.shape[-1] > 1):
            x, y = x.reshape(x.shape[0], self.N), y.reshape(x.shape[0], self.N)
        return _lib.require_gpu_tensor(x, "x"), _lib.require_gpu_tensor(y, "y")

    def _call_cost(self, cost_matrix, x):
        """``forward(..., cost_matrix=)``: an ``(N, N)`` or ``(B, N, N)`` f32 device tensor that stands in for the
        module's matrix for one call, as ``(M, Mt)``."""
        M = _lib.require_gpu_tensor(cost_matrix, "cost_matrix")
        B = x.shape[0]
        if tuple(M.shape) not in ((self.N, self.N), (B, self.N, self.N)):
            raise ValueError("cost_matrix must be (N, N) or (B, N, N) with B = %d, N = %d; got %s"
                             % (B, self.N, tuple(M.shape)))
        return M, M.transpose(-1, -2).contiguous()

    def _cost_and_range(self, x, y, cost_matrix=None):
        """The cost matrices on the samples' device and, under ``sync_diameter``, the range of the global batch
        (``(2,)``, or ``(2*D,)`` for D > 1)."""
        M, Mt = self.cost_matrix(x.device) if cost_matrix is None else self._call_cost(cost_matrix, x)
        return M, Mt, global_range(x, y) if (self.sync_diameter and self.diameter is None) else None

    def forward(self, *args, cost_matrix=None):
        """``cost_matrix``: an ``(N, N)`` or per-sample ``(B, N, N)`` f32 device tensor used instead of the module's
        matrix for this call (no gradient reaches it: the reference detaches M, ``gmloss/utils.py:104``)."""
        a, x, b, y = self.process_args(*args)
        self._check_samples(x, y)
        x, y = self._samples(x, y)
        B = x.shape[0]
        if B == 0:
            return x.new_zeros(0) + 0.0 * (x.sum() + y.sum())
        a = None if a is None else _lib.require_gpu_tensor(a.reshape(B, self.N), "alpha")
        b = None if b is None else _lib.require_gpu_tensor(b.reshape(B, self.N), "beta")
        M, Mt, rng = self._cost_and_range(x, y, cost_matrix)
        return _SinkhornDivergence.apply(x, y, a, b, M, Mt, self.p, self.blur, self.scaling, self.diameter, rng, self.rho)

    def forward_raw(self, x, y, need_gx=True, need_gy=True, out=None, flags=None, want_lam=False, cost_matrix=None):
        """Every device output of one call (loss, unit grads, schedule, duals; with ``want_lam`` the dampening schedule
        ``lam`` next to ``eps_s``) -- for parity tests and timing.  1-D points may come as ``(B, N)`` or ``(B, N, 1)``;
        ``(B, N, D)`` samples with D > 1 give gradients ``(B, N, D)``.  ``cost_matrix``: as in ``forward``."""
        if x.dim() == 3 and x.shape[-1] > 1:
            self._check_samples(x, y)
        x, y = self._samples(x, y)
        M, Mt, rng = self._cost_and_range(x, y, cost_matrix)
        return sinkhorn_raw(x, y, None, None, M, Mt, self.p, self.blur, self.scaling, self.diameter,
                            need_gx, need_gy, out, range_lo_hi=rng, flags=flags, rho=self.rho, want_lam=want_lam)
