"""Projector inputs.  The reference's ``LavalIndoorDataset.__getitem__`` (``GenProjector/data.py:58-108``)
rasterises the ground-truth Gaussian map PER SAMPLE on the GPU inside the loader; here the whole batch is one
call of the HIP rasteriser (``eml_sg_rasterise_f32``) in the training step.  EXR I/O is out of scope; the
synthetic generator follows SURVEY 8d.

``ProjectorPanoramaBatcher`` makes the reference's per-sample dict from HDR panoramas on the device (``*.npy``, see
``RegressionNetwork.data.PanoramaDataset``): ``light_targets`` (``data.py:73-84``) and ``resize_bilinear`` (``data.py:70``)
are the two operators of csrc/projector_prep.hip, the rest is ``PanoramaBatcher``'s crop / area resize / tonemap,
``extract_mesh`` and the rasteriser.  ``resize_exr`` is the reference's panorama warp (``util.py:279-343``) on the device;
``warp=`` / ``move_range=`` of the batcher apply it to the 128 x 256 panorama, so ``warped`` and ``map`` are those of the
position the crop shows, as the reference's ``warpedHDROutputs`` files are (``data.py:73``)."""
import torch
import torch.nn.functional as F

from .. import _lib
from ..RegressionNetwork.data import PanoramaBatcher, synthetic_batch
from ..RegressionNetwork.util import PanoramaHandler, convert_to_panorama, sphere_points, tonemap_raw


_ANCHORS = {}


def anchor_dirs(ln, dev):
    """The Fibonacci anchors as a (1, 3 ln) device tensor, built once per (ln, device): the joint step calls ``gaussian_map`` every
    iteration, and a fresh ``torch.from_numpy(...).to(dev)`` there is a pageable host-to-device copy -- a host synchronisation
    in the middle of the step (round 6: every such copy on the iteration's path is gone, ``tools/capture_probe.py``)."""
    key = (int(ln), str(dev))
    if key not in _ANCHORS:
        _ANCHORS[key] = torch.from_numpy(sphere_points(ln)).float().view(1, ln * 3).to(dev)
    return _ANCHORS[key]


def gaussian_map(distribution, intensity, rgb_ratio, ambient, alpha=None, ln=128, pano_hw=(128, 256)):
    """``data.py:86-102``: light = dist * (intensity*0.01) * rgb per anchor, SG lobes of width .0025 on the
    Fibonacci anchors, + ambient / (H*W), * alpha.  All arguments are batched device tensors."""
    B = distribution.shape[0]
    dev = distribution.device
    dirs = anchor_dirs(ln, dev).expand(B, -1).contiguous()
    size = torch.full((B, ln), 0.0025, device=dev)
    light = (distribution.view(B, ln, 1) * (intensity.view(B, 1, 1) * 0.01) * rgb_ratio.view(B, 1, 3))
    env = convert_to_panorama(dirs, size, light.reshape(B, ln * 3).contiguous(), pano_hw=pano_hw)
    env = env + (ambient / (pano_hw[0] * pano_hw[1])).view(B, 3, 1, 1)
    return env if alpha is None else env * alpha.view(B, 1, 1, 1)


def projector_batch(batch, device, ln=128, pano_hw=(128, 256), seed=1234):
    """Synthetic ``{'input','crop','warped','map'}`` batch on ``device``."""
    p = synthetic_batch(batch, ln, (128, 128), seed=seed, device=device)
    g = torch.Generator().manual_seed(seed + 7)
    inp = gaussian_map(p["distribution"], p["intensity"] * 500.0, p["rgb_ratio"], p["ambient"] * pano_hw[0] * pano_hw[1],
                       ln=ln, pano_hw=pano_hw)
    noise = F.interpolate(torch.empty(batch, 1, 8, 16).uniform_(0.5, 1.5, generator=g), size=pano_hw,
                          mode="bilinear", align_corners=False).to(device)
    warped = inp * noise
    luma = 0.3 * warped[:, 0] + 0.59 * warped[:, 1] + 0.11 * warped[:, 2]
    mask = (luma > 0.05 * luma.amax(dim=(1, 2), keepdim=True)).float().unsqueeze(1)
    return {"input": inp, "crop": p["crop"], "warped": warped, "map": mask}


def _alpha_arg(alpha, B):
    if alpha is None:
        return None
    a = _lib.require_gpu_tensor(alpha, "alpha")
    if a.shape != (B,):
        raise ValueError("alpha: expected one value per sample, shape (%d,), got %s" % (B, tuple(a.shape)))
    return a


def light_targets(small, alpha=None):
    """``data.py:73-84`` for a batch (``eml_projector_targets_f32``): ``small`` ``(B, h, w, 3)`` float32, pixel-major as
    ``PanoramaHandler.resize_panorama`` writes it, ``alpha`` ``(B,)`` or ``None`` for 1 -> ``warped`` ``(B, 3, h, w)`` =
    ``small * alpha`` channel-first and ``map`` ``(B, 1, h, w)`` in {0, 1} = luma > 5 % of the image's largest luma, the luma
    formed in float32 in the reference's association.  Device tensors only; run-to-run exact."""
    x = _lib.require_gpu_tensor(small, "small")
    if x.dim() != 4 or x.shape[3] != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("small: expected (B, h, w, 3) with h, w >= 1, got %s" % (tuple(x.shape),))
    B, h, w, _ = x.shape
    a = _alpha_arg(alpha, B)
    L = _lib.lib()
    warped = torch.empty(B, 3, h, w, dtype=torch.float32, device=x.device)
    mask = torch.empty(B, 1, h, w, dtype=torch.float32, device=x.device)
    if B == 0:
        return warped, mask
    work = torch.empty(max(1, L.eml_projector_targets_work_floats(B, h, w)), dtype=torch.float32, device=x.device)
    _lib.check(L.eml_projector_targets_f32(_lib.ptr(x), _lib.ptr(a), B, h, w, _lib.ptr(warped), _lib.ptr(mask), _lib.ptr(work),
                                           _lib.current_stream()), "eml_projector_targets_f32")
    return warped, mask


def resize_bilinear(x, size, alpha=None, clip=False):
    """``cv2.resize(img, (w, h))`` with its default ``INTER_LINEAR`` (``data.py:70``) for a channel-first batch
    (``eml_resize_bilinear_f32``): ``x`` ``(B, C, h, w)`` float32 -> ``(B, C, size[0], size[1])``, the formula of
    ``F.interpolate(mode="bilinear", align_corners=False)`` with float64 positions, no antialiasing.  ``alpha`` ``(B,)``
    scales every tap and ``clip`` clamps it to [0, 1] first: with the tonemap's ``P`` and ``alpha`` the result is the resized
    tonemapped image.  Device tensors only; no gradient.  Parity with cv2 is by formula, not tested (cv2 was not available)."""
    x = _lib.require_gpu_tensor(x, "x")
    if x.dim() != 4 or min(x.shape[1:]) < 1:
        raise ValueError("x: expected a non-empty (B, C, h, w) batch, got %s" % (tuple(x.shape),))
    oh, ow = int(size[0]), int(size[1])
    if oh < 1 or ow < 1:
        raise ValueError("size must be (h, w) >= 1, got %r" % (size,))
    B, C, h, w = x.shape
    a = _alpha_arg(alpha, B)
    out = torch.empty(B, C, oh, ow, dtype=torch.float32, device=x.device)
    if B == 0:
        return out
    _lib.check(_lib.lib().eml_resize_bilinear_f32(_lib.ptr(x), _lib.ptr(a), 1 if clip else 0, B, C, h, w, oh, ow, _lib.ptr(out),
                                                  _lib.current_stream()), "eml_resize_bilinear_f32")
    return out


def resize_exr(img, res_x=512, res_y=512, theta=0.0, phi=0.0, move=0.0):
    """The reference's ``resize_exr(img, res_x, res_y)`` (``GenProjector/util.py:279-343``) on device tensors, one image
    ``(H, W, 3)`` or a batch: ``res_x`` is the number of ROWS of the result and ``res_y`` its columns, as there; the three
    constants of ``util.py:281`` are keywords (degrees, degrees, sphere radii; numbers or ``(B,)`` device tensors).  Differentiable
    (once) in the image and in parameter tensors that require grad.  See ``PanoramaHandler.warp_panorama``."""
    return PanoramaHandler.warp_panorama(img, (int(res_y), int(res_x)), theta=theta, phi=phi, move=move)


class ProjectorPanoramaBatcher(PanoramaBatcher):
    """Device panoramas ``(B, H, W, 3)`` -> the dict of the reference's ``LavalIndoorDataset.__getitem__``
    (``GenProjector/data.py:58-108``), the whole batch at once:

    * ``input`` ``(B, 3, 128, 256)``: ``gaussian_map`` of the ``extract_mesh(ln=anchors)`` parameters of ``pano``, times alpha
      (``data.py:86-102``);
    * ``crop`` ``(B, 3, 128, 128)``: ``TonemapHDR(2.4, 50, 0.5)`` of the perspective crop, resized (``data.py:69-70``) -- the
      resize takes the tonemap's ``P`` and ``alpha``, the full-size tonemapped crop is not made;
    * ``warped`` ``(B, 3, 128, 256)``, ``map`` ``(B, 1, 128, 256)``: ``light_targets(pano, alpha)`` (``data.py:73-84``);
    * ``pano`` ``(B, 128, 256, 3)``: the rotated panorama area-resized (and warped, if asked), ``alpha`` ``(B,)``: the crop's tonemap alpha.

    Views are drawn exactly as ``PanoramaBatcher`` draws them (same generator and seed, one azimuth per sample, the rotation
    folded into the gathers), so ``warped`` is the panorama centred on the crop's viewing direction, seen from the camera's
    own position.  The reference reads a panorama warped offline to the position the crop shows instead (``data.py:73``);
    that operator is ``resize_exr`` (``GenProjector/util.py:279-343``): ``warp=`` / ``move_range=`` (see ``PanoramaBatcher``)
    apply it to the 128 x 256 panorama before ``extract_mesh`` and ``light_targets``, the crop is untouched.
    ``regression=True`` adds ``PanoramaBatcher``'s ``distribution, intensity, rgb_ratio, ambient``; ``crop`` is then the
    full-size tonemapped crop the encoder reads and the 128 x 128 one goes under ``crop128`` (``JointTrainer`` uses it).
    The call only enqueues work."""

    CROP128 = (128, 128)

    def __init__(self, anchors=128, crop_hw=(192, 256), fov_deg=60.0, device="cuda", seed=1234, regression=False, mesh=None,
                 move_range=None):
        super().__init__(anchors=anchors, crop_hw=crop_hw, fov_deg=fov_deg, device=device, seed=seed, mesh=mesh,
                         move_range=move_range)
        self.regression = bool(regression)

    def __call__(self, panos, deg=None, fov_deg=None, warp=None):
        deg, fov = self.view(panos, deg, fov_deg)
        warp = self.warp_of(panos, warp)
        raw = tonemap_raw(self.crop(panos, deg, fov), self.tone.gamma, self.tone.percentile, self.tone.max_mapping, clip=True,
                          apply=self.regression)
        alpha = raw["alpha"].contiguous()
        crop128 = resize_bilinear(raw["P"], self.CROP128, alpha=alpha, clip=True)
        small = self.warped(self.small(panos, deg), warp)
        para, _ = self.mesh.compute(small)
        warped, mask = light_targets(small, alpha)
        out = {"input": gaussian_map(para["distribution"].float(), para["intensity"].float(), para["rgb_ratio"].float(),
                                     para["ambient"].float(), alpha, ln=self.anchors, pano_hw=self.PANO_HW),
               "crop": crop128, "warped": warped, "map": mask, "pano": small, "alpha": alpha}
        if self.regression:
            out.update(self.targets(para, alpha), crop=raw["out"], crop128=crop128)
        return out
