"""CPU: ``--pano_dir DIR [--fov F]`` on the projector's and the joint entry points -- the reference's own command line
(``train_laval.sh``'s argv, restated from ``test_projector_cli.py``) still parses, its dataset flags are named as ignored,
and without ``--pano_dir`` and ``--synthetic`` the refusal is what it was."""
import numpy as np
import pytest
import torch

from emlight_amd import joint
from emlight_amd.GenProjector import options
from emlight_amd.GenProjector import test as gp_test
from emlight_amd.GenProjector import train as gp_train

TRAIN_LAVAL_SH = ["--name", "lavalindoor", "--dataset_mode", "lavalindoor", "--dataroot",
                  "/home/fangneng.zfn/datasets/LavalIndoor/tpami/", "--display_freq", "1000", "--batchSize", "16", "--niter", "100",
                  "--niter_decay", "100", "--gpu_ids", "0,1", "--continue_train"]
TEST_SH = ["--name", "lavalindoor", "--checkpoints_dir", "./checkpoints", "--which_epoch", "100", "--dataset_mode", "lavalindoor",
           "--dataroot", "/home/fangneng.zfn/datasets/LavalIndoor/test/"]


def test_train_laval_sh_argv_with_pano_dir_under_a_two_rank_launch(monkeypatch, capsys, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    args = gp_train.parse_args(TRAIN_LAVAL_SH + ["--pano_dir", str(tmp_path)])
    assert args.pano_dir == str(tmp_path) and args.fov == 60.0 and not args.synthetic
    assert (args.name, args.batchSize, args.niter, args.niter_decay, args.continue_train) == ("lavalindoor", 16, 100, 100, True)
    assert set(args.ignored_reference_flags) == {"dataset_mode", "dataroot"}
    said = capsys.readouterr().out
    assert "accepted and ignored" in said and "--pano_dir" in said and "--dataset_mode" in said and "--dataroot" in said
    assert gp_train.parse_args(TRAIN_LAVAL_SH + ["--pano_dir", str(tmp_path), "--fov", "75"]).fov == 75.0
    monkeypatch.setenv("RANK", "1")                                    # one rank says it
    capsys.readouterr()
    gp_train.parse_args(TRAIN_LAVAL_SH + ["--pano_dir", str(tmp_path)])
    assert capsys.readouterr().out == ""


def test_test_and_joint_parsers_accept_pano_dir(monkeypatch, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = gp_test.parse_args(TEST_SH + ["--pano_dir", str(tmp_path), "--fov", "90"])
    assert args.pano_dir == str(tmp_path) and args.fov == 90.0 and args.which_epoch == "100"
    assert set(args.ignored_reference_flags) >= {"dataset_mode", "dataroot"}
    assert gp_test.parse_args(["--synthetic"]).pano_dir is None
    j = joint.build_parser().parse_args(["--pano_dir", str(tmp_path), "--fov", "45", "--batch", "4"])
    assert j.pano_dir == str(tmp_path) and j.fov == 45.0 and j.batch == 4
    d = joint.build_parser().parse_args([])
    assert d.pano_dir is None and (d.batch, d.anchors, tuple(d.crop_hw), d.max_iters) == (32, 128, (240, 320), 100)


def test_the_refusal_without_either_flag_is_unchanged(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        gp_train.parse_args(TRAIN_LAVAL_SH)
    assert str(e.value) == (
        "GenProjector: the Laval dataset reader (--dataset_mode lavalindoor, --dataroot "
        "/home/fangneng.zfn/datasets/LavalIndoor/tpami/) is outside this package (SURVEY 8b: the data loader is the caller's): "
        "pass --synthetic for the seeded synthetic batches of SURVEY 8d, or feed `Trainer.step` your own batches "
        "{input, crop, warped, map}")
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit) as e:
        gp_test.parse_args(TEST_SH)
    assert "--synthetic" in str(e.value) and "lavalindoor" in str(e.value)
    # --synthetic keeps its own line
    ap = options.train_parser()
    args = ap.parse_args(["--synthetic", "--dataset_mode", "lavalindoor"])
    assert options.check_data_flags(args, ap, True, verbose=False) == ["dataset_mode"]


def test_pano_loader_is_the_regression_trainers_arrangement(tmp_path):
    """One epoch is one pass over the directory: the loader drops the ragged last batch, ``IterationCounter`` gets len(dataset)."""
    from emlight_amd.GenProjector.iter_counter import IterationCounter
    args = gp_train.parse_args(["--pano_dir", str(tmp_path), "--batchSize", "2"])
    with pytest.raises(FileNotFoundError):
        gp_train.make_pano_loader(args, "cpu", 0, 1)
    np.save(str(tmp_path / "a.npy"), np.zeros((8, 16, 3), dtype=np.float32))
    with pytest.raises(SystemExit, match="fewer than one global batch"):
        gp_train.make_pano_loader(args, "cpu", 0, 1)
    assert gp_train.make_pano_loader(gp_train.parse_args(["--synthetic"]), "cpu", 0, 1) == (None, None, None)
    counter = IterationCounter(str(tmp_path), "x", 3, 2, niter=1)
    assert counter.dataset_size == 3
