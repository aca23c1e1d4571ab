#!/usr/bin/env python
"""Generate tests/golden/panorama_prep.npz by running the REAL reference on seeded inputs (CPU).

Run only where the reference checkout exists (see ``make_golden.py``):

    python tests/golden/make_golden_panorama.py

The reference's ``RegressionNetwork/util.py`` holds unresolved merge markers and does not import; its text is read at
generation time, the marker lines are dropped and the rest is executed -- nothing of it is stored.  That gives the
reference's ``PanoramaHandler`` (crop, rotate) and the ``TonemapHDR`` that returns ``(img, alpha)``.  Absent third-party
modules are stubbed as in ``make_golden.py``.  The file holds OUTPUTS only; the inputs are the seeded recipes below,
which the tests import.

Two places where the stored chain is not the reference's call, both because ``cv2`` is not installed:
* the 128 x 256 panorama handed to ``extract_mesh`` is the box mean of the rotated panorama (float64 mean, rounded to
  float32), where the reference calls ``cv2.resize(..., INTER_AREA)``;
* the reference cuts its crops offline and reads them back from float32 EXR files; the batcher items round the
  reference's float64 crop to float32 before the tonemap, as that file format would.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))

DEGS = (0.0, 77.3, -45.0, 359.9, 720.5)

# name, (H, W), seed, fov, crop_image_h, aspect, deg, uint8 input
CROP_CASES = [("big_fov%d" % fov, (256, 512), 11, float(fov), 48, "4:3", DEGS[i % 5], False)
              for i, fov in enumerate((40, 60, 90, 120, 150, 170))]
CROP_CASES += [("small_deg%d" % i, (64, 128), 12, float(fov), 24, "4:3", deg, False)
               for i, (deg, fov) in enumerate(zip(DEGS, (60, 170, 40, 120, 90)))]
CROP_CASES += [("small_u8", (64, 128), 13, 90.0, 24, "4:3", 77.3, True),
               ("small_16_9", (64, 128), 12, 60.0, 24, "16:9", -45.0, False),
               ("big_h24_150", (256, 512), 11, 150.0, 24, "4:3", 359.9, False)]
# leaves the interpolator's grid: the reference raises ValueError (elevation beyond row H - 1)
CROP_OUT_OF_BOUNDS = ("oob", (64, 128), 12, 170.0, 26, "1:2", 0.0, False)   # w = 13: the middle column is X = 0

TONE_SETTINGS = [(2.4, 50, .5), (2.4, 99, .99), (2.4, 99, .9), (1., 90, .8)]   # the four the reference uses
# name, input kind, setting index, kwargs of __call__
TONE_CASES = [("set%d" % i, "heavy", i, {}) for i in range(4)]
TONE_CASES += [("nogamma", "heavy", 0, {"gamma": False}),
               ("alpha", "heavy", 0, {"alpha": 0.37}),
               ("zero_band", "zero_band", 0, {}),
               ("all_zero", "all_zero", 0, {}),
               ("noclip", "heavy", 1, {"clip": False})]
TONE_HW = (24, 32)

BATCHER = {"B": 2, "HW": (256, 512), "seed": 21, "deg": (77.3, -45.0), "fov": 60.0, "crop_hw": (24, 32), "anchors": 96}


def rng(*seed):
    return np.random.default_rng(list(seed))


def pano_inputs(B, H, W, seed, uint8=False):
    """Heavy-tailed radiance (B, H, W, 3) f32: U^8 * 50 with three saturated light patches in the thousands per image;
    ``uint8``: an 8-bit image instead."""
    g = rng(seed, B, H, W)
    if uint8:
        return g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    out = g.random((B, H, W, 3)) ** 8 * 50.0
    for b in range(B):
        for _ in range(3):
            ph, pw = max(1, H // 16), max(1, W // 16)
            y0, x0 = int(g.integers(0, H - ph)), int(g.integers(0, W - pw))
            out[b, y0:y0 + ph, x0:x0 + pw] = g.uniform(1000, 5000) * g.uniform(0.5, 1.0, 3)
    return out.astype(np.float32)


def tone_inputs(kind, seed=31):
    """One radiance image (3, h, w) f32 for the tonemap cases."""
    h, w = TONE_HW
    img = np.ascontiguousarray(pano_inputs(1, h, w, seed)[0].transpose(2, 0, 1))
    if kind == "zero_band":
        img[:, 8:16] = 0.0
    elif kind == "all_zero":
        img[:] = 0.0
    elif kind != "heavy":
        raise ValueError(kind)
    return img


def box_mean(pano, h, w):
    """(H, W, 3) -> (h, w, 3): mean of each (H/h) x (W/w) box in float64, rounded to float32."""
    H, W, _ = pano.shape
    return pano.astype(np.float64).reshape(h, H // h, w, W // w, 3).mean(axis=(1, 3)).astype(np.float32)


def ref_util():
    """The reference's RegressionNetwork/util.py, executed from its text without the merge-marker lines."""
    from make_golden import REF, stub_io_modules
    stub_io_modules()
    path = os.path.join(REF, "RegressionNetwork", "util.py")
    lines = [ln for ln in open(path).read().split("\n") if not ln.startswith(("<<<<<<<", "=======", ">>>>>>>"))]
    ns = {"__name__": "ref_regression_util"}
    exec(compile("\n".join(lines), path, "exec"), ns)
    return ns


def main():
    import torch
    from make_golden import ref_extract_mesh
    ns = ref_util()
    handler, Tone = ns["PanoramaHandler"], ns["TonemapHDR"]
    out = {}
    for name, (H, W), seed, fov, h, aspect, deg, u8 in CROP_CASES:
        pano = pano_inputs(1, H, W, seed, uint8=u8)[0]
        crop = handler.crop_panorama(handler.horizontal_rotate_panorama(pano, deg), fov, h, aspect)
        out["crop/%s" % name] = np.ascontiguousarray(crop.transpose(2, 0, 1)).astype(np.float32)   # f64 -> nearest f32
        print("crop", name, crop.shape, "max %.1f" % crop.max())
    name, (H, W), seed, fov, h, aspect, deg, u8 = CROP_OUT_OF_BOUNDS
    try:
        handler.crop_panorama(pano_inputs(1, H, W, seed)[0], fov, h, aspect)
        raised = False
    except ValueError:
        raised = True
    assert raised, "the out-of-bounds case must raise in the reference"
    out["crop/%s/raises" % name] = np.bool_(raised)

    for name, kind, si, kw in TONE_CASES:
        img, alpha = Tone(*TONE_SETTINGS[si])(tone_inputs(kind), **kw)
        out["tone/%s/out" % name] = img
        out["tone/%s/alpha" % name] = np.float64(alpha)
        print("tone", name, img.dtype, "alpha %.6g" % alpha)

    cfg = BATCHER
    panos = pano_inputs(cfg["B"], cfg["HW"][0], cfg["HW"][1], cfg["seed"])
    mesh = ref_extract_mesh()(h=128, w=256, ln=cfg["anchors"])
    tone = Tone(gamma=2.4, percentile=50, max_mapping=0.5)                      # data.py:43
    h, w = cfg["crop_hw"]
    for b in range(cfg["B"]):
        rot = handler.horizontal_rotate_panorama(panos[b], cfg["deg"][b])
        crop = handler.crop_panorama(rot, cfg["fov"], h, "%d:%d" % (w // 8, h // 8)).astype(np.float32)
        img, alpha = tone(crop)                                                 # data.py:63
        para, _ = mesh.compute(box_mean(rot, 128, 256))
        out["batch/%d/crop" % b] = np.ascontiguousarray(img.transpose(2, 0, 1))           # ToTensor, data.py:64
        out["batch/%d/alpha" % b] = np.float64(alpha)
        out["batch/%d/distribution" % b] = np.asarray(para["distribution"], dtype=np.float64)
        out["batch/%d/rgb_ratio" % b] = np.asarray(para["rgb_ratio"], dtype=np.float64)
        out["batch/%d/intensity_raw" % b] = np.float64(para["intensity"])
        out["batch/%d/ambient_raw" % b] = np.asarray(para["ambient"], dtype=np.float64)
        # data.py:71,73
        out["batch/%d/intensity" % b] = (torch.from_numpy(np.array(para["intensity"])).float() * alpha / 500).numpy()
        out["batch/%d/ambient" % b] = (torch.from_numpy(para["ambient"]).float() * alpha / (128 * 256)).numpy()
        print("batch", b, "alpha %.6g" % alpha, "intensity", out["batch/%d/intensity" % b])
    path = os.path.join(HERE, "panorama_prep.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
