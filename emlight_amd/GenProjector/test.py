"""Entry point mirroring ``GenProjector/test.py:20-38``: load ``<which_epoch>_net_G.pth``, run the generator in
inference mode on each batch, write the predicted HDR panoramas as ``.npy`` (EXR writing is out of scope).

    python -m emlight_amd.GenProjector.test --synthetic --how_many 4
    python -m emlight_amd.GenProjector.test --pano_dir DIR --name lavalindoor      # pred_<name>.npy per panorama, view at azimuth 0
"""
import argparse
import os

import numpy as np
import torch

from . import data, networks, options
from .pix2pix_model import Pix2PixModel


def parse_args(argv=None):
    """The reference's flags (``options/test_options.py`` over ``base_options.py``: ``test.sh`` runs unchanged) + ``--synthetic``
    and ``--pano_dir --fov``."""
    ap = options.test_parser()
    args = ap.parse_args(argv)
    args.gpu_id_list = options.resolve_gpu_ids(args.gpu_ids, 1)
    args.ignored_reference_flags = options.check_data_flags(args, ap, args.synthetic, pano_dir=args.pano_dir)
    return args


def run_panoramas(args, model, dev):
    """``--pano_dir``: every panorama of the directory in name order, the view at azimuth 0 (inference is repeatable), one
    ``pred_<name>.npy`` ``(1, 3, 128, 256)`` each; ``--how_many`` bounds the number of batches as in the reference."""
    from torch.utils.data import DataLoader
    from ..RegressionNetwork.data import PanoramaDataset
    loader = DataLoader(PanoramaDataset(args.pano_dir), batch_size=args.batchSize, shuffle=False, drop_last=False)
    batcher = data.ProjectorPanoramaBatcher(fov_deg=args.fov, device=dev)
    for i, para in enumerate(loader):
        if i >= args.how_many:
            break
        fake = model(batcher(para["pano"].to(dev), deg=0.0), mode="inference").cpu().numpy()
        for j, name in enumerate(para["name"]):
            np.save(os.path.join(args.results_dir, "pred_%s.npy" % name), fake[j:j + 1])
            print("process image... %s" % name)


def main(argv=None):
    from emlight_amd import _runtime
    _runtime.entry_point_defaults()   # kernel arguments in device memory, recorded library-GEMM selection: an entry point's choice
    args = parse_args(argv)
    dev = "cuda:%d" % args.gpu_id_list[0]
    opt = options.network_options(args, False)
    model = Pix2PixModel(opt).to(dev).eval()
    path = os.path.join(args.checkpoints_dir, args.name, "%s_net_G.pth" % args.which_epoch)
    if os.path.exists(path):
        model.netG.load_state_dict(torch.load(path, map_location=dev))
    os.makedirs(args.results_dir, exist_ok=True)
    if args.pano_dir:
        return run_panoramas(args, model, dev)
    # the reference stops after 1000 samples (test.py:23-25); the synthetic stream is endless, so --how_many bounds it (default 10)
    how_many = 10 if args.how_many == float("inf") else int(args.how_many)
    for i in range(how_many):
        batch = data.projector_batch(args.batchSize, dev, seed=4321 + i)
        fake = model(batch, mode="inference")
        np.save(os.path.join(args.results_dir, "pred_%04d.npy" % i), fake.cpu().numpy())
        print("process image... %d" % i)


if __name__ == "__main__":
    main()
