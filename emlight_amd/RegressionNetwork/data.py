"""Datasets for the regression network.

The reference's ``ParameterDataset`` (``RegressionNetwork/data.py:20-87``) reads the
licence-restricted Laval Indoor EXR crops + pickled GT parameters; that I/O is out of scope
(SURVEY C7).  ``SyntheticParameterDataset`` yields the same dict -- keys ``crop``,
``distribution``, ``intensity``, ``rgb_ratio``, ``ambient``, ``name`` with the same shapes
and value ranges -- from a seeded generator, and ``PickleParameterDataset`` reads the
reference's on-disk format (``representation/distribution_representation.py:116-119``)
when a directory of ``*.pickle`` + ``*.npy`` crops is supplied.

``PanoramaDataset`` + ``PanoramaBatcher`` make the same dict from HDR panoramas on the device: a tonemapped
perspective crop at a chosen (or per-step random) azimuth and the four targets of ``extract_mesh`` scaled by the crop's
tonemap alpha -- the reference prepares both offline, one fixed view per panorama.
"""
import glob
import os
import pickle

import numpy as np
import torch
from torch.utils.data import Dataset


DEPTH_SEED_OFFSET = 7919   # the depth's own generator: seed + this, so the other tensors keep their bits


def synthetic_batch(batch, anchors=128, crop_hw=(240, 320), seed=1234, device="cpu", with_depth=False):
    """One seeded synthetic batch: uniform crops, sparse-simplex distribution
    (mimics the >5%-of-max light mask of ``distribution_representation.py:96,110``),
    intensity U(.05,2), unit-L2 rgb ratio, ambient U(0,.3).  ``with_depth``: also ``depth`` ``(batch, anchors)``, the
    per-anchor scene depth of ``gmloss.SamplesLoss`` (reference ``data.py:75``), U(.5, 3) from a generator of its own:
    every other tensor is the same with and without it."""
    g = torch.Generator().manual_seed(seed)
    crop = torch.rand(batch, 3, crop_hw[0], crop_hw[1], generator=g)
    d = torch.softmax(4.0 * torch.randn(batch, anchors, generator=g), dim=1)
    thr = torch.quantile(d, 0.75, dim=1, keepdim=True)
    d = torch.where(d < thr, torch.zeros_like(d), d)
    d = d / d.sum(1, keepdim=True)
    intensity = torch.empty(batch, 1).uniform_(0.05, 2.0, generator=g)
    rgb = torch.empty(batch, 3).uniform_(0.4, 0.7, generator=g)
    rgb = rgb / rgb.norm(dim=1, keepdim=True)
    ambient = torch.empty(batch, 3).uniform_(0.0, 0.3, generator=g)
    out = {"crop": crop, "distribution": d, "intensity": intensity, "rgb_ratio": rgb, "ambient": ambient}
    if with_depth:
        gd = torch.Generator().manual_seed(seed + DEPTH_SEED_OFFSET)
        out["depth"] = torch.empty(batch, anchors).uniform_(0.5, 3.0, generator=gd)
    return {k: v.to(device) for k, v in out.items()}


class SyntheticParameterDataset(Dataset):
    def __init__(self, length=4096, anchors=128, crop_hw=(240, 320), seed=1234, with_depth=False):
        self.length, self.anchors, self.crop_hw, self.seed = length, anchors, tuple(crop_hw), seed
        self.with_depth = bool(with_depth)

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        b = synthetic_batch(1, self.anchors, self.crop_hw, seed=self.seed + idx, with_depth=self.with_depth)
        item = {k: v[0] for k, v in b.items()}
        item["name"] = "synthetic_%06d" % idx
        return item


class PickleParameterDataset(Dataset):
    """``<dir>/<name>.pickle`` = {'distribution','intensity','rgb_ratio','ambient'} (the
    reference's GT format) next to ``<name>.npy`` = tonemapped crop (3,H,W) f32 in [0,1].
    Scaling follows ``data.py:70-73``: intensity*alpha/500, ambient*alpha/(128*256) with the
    tonemap alpha stored in the pickle as 'alpha' (1.0 if absent).  A pickle that holds 'depth' (the per-anchor scene
    depth, ``data.py:75``) gives a ``depth`` item ``(N,)`` f32 as well; without it the key is absent."""

    def __init__(self, root):
        self.items = sorted(glob.glob(os.path.join(root, "*.pickle")))
        if not self.items:
            raise FileNotFoundError("no *.pickle under %s" % root)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        path = self.items[idx]
        with open(path, "rb") as f:
            p = pickle.load(f)
        alpha = float(p.get("alpha", 1.0))
        crop = np.load(path[:-len(".pickle")] + ".npy").astype(np.float32)
        item = {"crop": torch.from_numpy(crop),
                "distribution": torch.as_tensor(p["distribution"], dtype=torch.float32),
                "intensity": torch.as_tensor(p["intensity"], dtype=torch.float32).reshape(1) * alpha / 500.0,
                "rgb_ratio": torch.as_tensor(p["rgb_ratio"], dtype=torch.float32),
                "ambient": torch.as_tensor(p["ambient"], dtype=torch.float32) * alpha / (128 * 256),
                "name": os.path.basename(path)[:-len(".pickle")]}
        if "depth" in p:
            item["depth"] = torch.as_tensor(np.asarray(p["depth"]), dtype=torch.float32).reshape(-1)
        return item


class PanoramaDataset(Dataset):
    """``<root>/*.npy`` HDR panoramas ``(H, W, 3)`` (equirect, linear radiance), returned as float32 tensors with their
    names.  EXR input stays out of scope: convert offline.

    ``depth_dir``: every item also has ``depth_pano`` ``(H, W)`` float32 from ``<depth_dir>/<name>.npy``, the distance from the
    viewpoint to the scene along each pixel's direction (what ``PanoramaBatcher(depth_panos=...)`` takes).  A panorama
    without a depth file is a ``FileNotFoundError`` at construction; a depth of another shape, or with a value that is not
    finite or not > 0, is a ``ValueError`` naming the file when the item is read."""

    def __init__(self, root, depth_dir=None):
        self.items = sorted(glob.glob(os.path.join(root, "*.npy")))
        if not self.items:
            raise FileNotFoundError("no *.npy under %s" % root)
        self.depth_dir = depth_dir
        if depth_dir is not None:
            for path in self.items:
                if not os.path.isfile(self.depth_path(path)):
                    raise FileNotFoundError("%s has no depth panorama %s" % (path, self.depth_path(path)))

    def depth_path(self, path):
        return os.path.join(self.depth_dir, os.path.basename(path))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        path = self.items[idx]
        pano = np.load(path)
        if pano.ndim != 3 or pano.shape[2] != 3:
            raise ValueError("%s: expected a (H, W, 3) panorama, got %s" % (path, pano.shape))
        item = {"pano": torch.from_numpy(np.ascontiguousarray(pano, dtype=np.float32)),
                "name": os.path.basename(path)[:-len(".npy")]}
        if self.depth_dir is not None:
            dpath = self.depth_path(path)
            depth = np.load(dpath)
            if depth.shape != pano.shape[:2]:
                raise ValueError("%s: expected a depth panorama of shape %s like %s, got %s"
                                 % (dpath, pano.shape[:2], path, depth.shape))
            depth = np.ascontiguousarray(depth, dtype=np.float32)
            if not (np.isfinite(depth).all() and (depth > 0).all()):
                raise ValueError("%s: every depth must be finite and > 0" % dpath)
            item["depth_pano"] = torch.from_numpy(depth)
        return item


def add_warp_option(ap):
    """``--warp_move LO HI`` of the three train mains (valid with ``--pano_dir`` only, see ``warp_move_range``)."""
    ap.add_argument("--warp_move", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                    help="--pano_dir: derive the targets from the panorama warped to a position `move` sphere radii along the "
                         "view axis (negative: toward what the crop shows), one move per sample drawn uniformly in [LO, HI) "
                         "(PanoramaBatcher(move_range=...)); default: the camera's own position.  With --depth_dir (the "
                         "regression trainer) the warp follows the scene's depth and LO, HI are in the units of the depth")
    return ap


def warp_move_range(args):
    """The parsed ``--warp_move`` as ``move_range`` (``None`` without the flag); exits with a message where the flag cannot
    apply: without ``--pano_dir`` no panorama exists to warp."""
    if getattr(args, "warp_move", None) is None:
        return None
    if not getattr(args, "pano_dir", None):
        raise SystemExit("--warp_move applies to the batches made from --pano_dir panoramas; without --pano_dir there is no "
                         "panorama to warp")
    lo, hi = args.warp_move
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise SystemExit("--warp_move LO HI: finite values with LO <= HI, got %r %r" % (lo, hi))
    return (float(lo), float(hi))


class PanoramaBatcher:
    """Device panoramas ``(B, H, W, 3)`` -> the training dict of the reference's ``ParameterDataset`` (``data.py:46-84``):

    * ``crop``: ``TonemapHDR(2.4, 50, 0.5)`` (``data.py:43,63``) of the perspective crop at azimuth ``deg`` and field of view
      ``fov_deg``, ``(B, 3, h, w)``;
    * ``distribution`` / ``rgb_ratio``: ``extract_mesh(ln=anchors).compute`` of the rotated panorama area-resized to
      128 x 256; ``intensity * alpha / 500`` and ``ambient * alpha / (128 * 256)`` (``data.py:71,73``), float32;
    * ``alpha``: the crop's tonemap alpha ``(B,)``.

    ``deg=None`` draws one azimuth in [0, 360) per sample from a seeded generator that lives on the device; a Python
    number holds for the batch, a ``(B,)`` device tensor gives one per sample (likewise ``fov_deg``).  The call only
    enqueues work: no ``.item()``, no ``.cpu()``, no pageable copy.  ``mesh``: an ``extract_mesh`` (h=128, w=256) to share.

    ``warp=(theta, phi, move)`` (numbers, or a ``(B, 3)`` device tensor) warps the 128 x 256 panorama to another position
    before the targets are derived (``PanoramaHandler.warp_panorama``, the reference's ``resize_exr``); the crop is
    untouched.  ``move_range=(lo, hi)`` at construction draws one ``move`` per sample uniformly in [lo, hi) from the same
    generator, after the azimuth, with ``theta = phi = 0``; a ``warp=`` passed to the call wins.  With neither, the calls made
    and every output are what they were without the arguments."""

    PANO_HW = (128, 256)

    def __init__(self, anchors=96, crop_hw=(192, 256), fov_deg=60.0, device="cuda", seed=1234, mesh=None, move_range=None):
        from fractions import Fraction
        from .representation import extract_mesh
        from .util import TonemapHDR
        self.crop_h, self.crop_w = int(crop_hw[0]), int(crop_hw[1])
        fr = Fraction(self.crop_w, self.crop_h)
        self.aspect = "%d:%d" % (fr.numerator, fr.denominator)
        if int(self.crop_h * (fr.numerator / fr.denominator)) != self.crop_w:   # the reference's w = int(h * ratio)
            raise ValueError("crop_hw %s: int(h * ratio) does not give back w" % (tuple(crop_hw),))
        self.anchors, self.fov_deg, self.device, self.seed = anchors, fov_deg, torch.device(device), seed
        self.mesh = mesh if mesh is not None else extract_mesh(h=self.PANO_HW[0], w=self.PANO_HW[1], ln=anchors, device=device)
        self.tone = TonemapHDR(gamma=2.4, percentile=50, max_mapping=0.5)
        self.generator = None   # made on the device at the first random draw
        if move_range is not None:
            if len(move_range) != 2 or not (np.isfinite(move_range[0]) and np.isfinite(move_range[1]) and move_range[0] <= move_range[1]):
                raise ValueError("move_range must be (lo, hi), finite, lo <= hi; got %r" % (move_range,))
            move_range = (float(move_range[0]), float(move_range[1]))
        self.move_range = move_range

    def _rand(self, B):
        if self.generator is None:
            self.generator = torch.Generator(device=self.device)
            self.generator.manual_seed(self.seed)
        return torch.rand(B, generator=self.generator, device=self.device, dtype=torch.float64)

    def random_deg(self, B):
        return self._rand(B) * 360.0

    def random_move(self, B):
        """One ``move`` per sample, uniform in ``move_range``, from the batcher's generator."""
        lo, hi = self.move_range
        return lo + self._rand(B) * (hi - lo)

    def warp_of(self, panos, warp=None):
        """The batch's warp as ``warp_panorama`` takes it: ``None`` (no warp) or ``(theta, phi, move)``, each a number or a
        ``(B,)`` device tensor.  Call it after ``view``: a drawn ``move`` comes after the azimuth in the generator's sequence."""
        B = panos.shape[0]
        if warp is None:
            return None if self.move_range is None else (0.0, 0.0, self.random_move(B))
        if isinstance(warp, torch.Tensor):
            if warp.shape != (B, 3):
                raise ValueError("warp: expected (theta, phi, move) per sample, shape (%d, 3), got %s" % (B, tuple(warp.shape)))
            return warp.unbind(1)
        if len(warp) != 3:
            raise ValueError("warp: expected (theta, phi, move), got %r" % (warp,))
        return tuple(float(v) for v in warp)

    def warped(self, small, warp):
        """``small`` warped to the position ``warp`` stands for; ``small`` itself without one."""
        if warp is None:
            return small
        from .util import PanoramaHandler
        return PanoramaHandler.warp_panorama(small, None, theta=warp[0], phi=warp[1], move=warp[2])

    def view(self, panos, deg=None, fov_deg=None):
        """The batch's ``(deg, fov_deg)``: what was passed, else one drawn azimuth per sample and the constructor's field of
        view.  ``GenProjector.data.ProjectorPanoramaBatcher`` draws its views through this, so the two agree."""
        if panos.dim() != 4:
            raise ValueError("expected panoramas (B, H, W, 3), got %s" % (tuple(panos.shape),))
        if deg is None:
            deg = self.random_deg(panos.shape[0])
        return deg, (self.fov_deg if fov_deg is None else fov_deg)

    def crop(self, panos, deg, fov):
        """The raw (HDR) perspective crop ``(B, 3, h, w)`` of the view."""
        from .util import PanoramaHandler
        return PanoramaHandler.crop_panorama(panos, fov, self.crop_h, self.aspect, deg=deg)

    def small(self, panos, deg):
        """The rotated panorama area-resized to 128 x 256, ``(B, 128, 256, 3)``."""
        from .util import PanoramaHandler
        return PanoramaHandler.resize_panorama(panos, (self.PANO_HW[1], self.PANO_HW[0]), deg=deg)

    @staticmethod
    def targets(para, alpha):
        """``extract_mesh.compute``'s parameters -> the four float32 regression targets (``data.py:70-73``)."""
        return {"distribution": para["distribution"].float(),
                "intensity": (para["intensity"].float() * alpha / 500.0).reshape(-1, 1),
                "rgb_ratio": para["rgb_ratio"].float(),
                "ambient": para["ambient"].float() * alpha[:, None] / (128 * 256)}

    def small_depth(self, panos, depth_panos, deg):
        """The depth panoramas ``(B, H, W)`` rotated and area-resized to 128 x 256 like the panoramas, ``(B, 128, 256)``: the
        same resize entry on a three-channel view of the depth (a copy of 3 H W floats per sample; no second resize kernel)."""
        if not isinstance(depth_panos, torch.Tensor) or depth_panos.shape != panos.shape[:3]:
            raise ValueError("depth_panos: expected %s like the panoramas, got %s"
                             % (tuple(panos.shape[:3]), tuple(getattr(depth_panos, "shape", ()))))
        return self.small(depth_panos.unsqueeze(-1).expand(-1, -1, -1, 3).contiguous(), deg)[..., 0].contiguous()

    def __call__(self, panos, deg=None, fov_deg=None, warp=None, depth_panos=None):
        """``depth_panos`` ``(B, H, W)`` float32, the scene's distance along each pixel of ``panos``: the result gains ``depth``
        ``(B, anchors)`` float32, the per-anchor depth GMLight's loss takes (``extract_mesh.anchor_depth``), and a warp becomes
        the parallax-correct one (``PanoramaHandler.warp_panorama_depth``) with ``move`` in the units of the depth: targets and
        depth are then those of the new position.  Without it the calls made and every output are what they were."""
        deg, fov = self.view(panos, deg, fov_deg)
        warp = self.warp_of(panos, warp)
        crop, alpha = self.tone(self.crop(panos, deg, fov))
        small = self.small(panos, deg)
        if depth_panos is None:
            para, _ = self.mesh.compute(self.warped(small, warp))
            return {"crop": crop, **self.targets(para, alpha), "alpha": alpha}
        depth = self.small_depth(panos, depth_panos, deg)
        if warp is not None:
            from .util import PanoramaHandler
            small, depth = PanoramaHandler.warp_panorama_depth(small, depth, None, theta=warp[0], phi=warp[1], move=warp[2])
        para, _ = self.mesh.compute(small)
        return {"crop": crop, **self.targets(para, alpha), "depth": self.mesh.anchor_depth(depth).float(), "alpha": alpha}
