"""Sequence evaluation (csrc/seq_eval.h mn_seq_windows, pgo.optimize_windows_dev, evaluate.predict_frames / evaluate_sequence,
scripts/eval.py --sequence): every frame forwarded once, the windows, their VOs and the pose-graph optimisation assembled on the device
from one pose per frame.  The checks are in tests/seq_eval_checks.py; CPU tests run the kernels in the SIMT emulator, the GPU tests
(-m gpu) on libmapnet_hip.so.  The bounds guard is exercised in the emulator only."""
import configparser
import os
import sys

import numpy as np
import pytest
import torch

import emu_lib
import seq_eval_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


@pytest.fixture(scope="module")
def hip():
    from geomapnet_amd import _binding
    assert torch.cuda.is_available()
    b = _binding.hip()
    assert b.backend_name == "hip"
    return b


_IDS = ["W%d-N%d-%s" % (w, n, "fc" if fc else "chain") for w, n, fc in K.OP_CASES]
PGO_CASES = ((3, False), (4, True))
_PGO_IDS = ["steps3-chain", "steps4-fc"]


# ---- operators: CPU suite (SIMT emulator) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,N,fc", K.OP_CASES, ids=_IDS)
def test_op_seq_windows(emu, W, N, fc):
    K.check_op_case(emu, "cpu", W, N, fc)


def test_op_seq_windows_clamped(emu):
    K.check_op_clamped(emu, "cpu")


def test_op_seq_windows_bounds_guard(emu):
    K.check_op_bounds_guard(emu, "cpu")


def test_op_seq_windows_errors(emu):
    K.check_op_errors(emu, "cpu")


def test_optimize_windows_dev(emu):
    K.check_optimize_windows_dev(emu, "cpu")


# ---- pose table and the loop: CPU suite ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fp32", "u8"])
def test_pose_table(emu, form):
    K.check_pose_table(emu, "cpu", "fp32", form)


def test_refusals(emu):
    K.check_refusals(emu, "cpu")


def test_against_loop(emu):
    K.check_against_loop(emu, "cpu", "fp32")


@pytest.mark.parametrize("steps,fc", PGO_CASES, ids=_PGO_IDS)
def test_against_loop_pose_graph(emu, steps, fc):
    K.check_against_loop_pose_graph(emu, "cpu", "fp32", steps, fc)


# ---- scripts/eval.py --sequence on the emulator -----------------------------------------------------------------------------------
H, W = 32, 40


def _eval_args(tmp_path, emu, config, extra, steps=3):
    import geomapnet_amd as G
    import eval as eval_script
    wfn = str(tmp_path / "w.pth.tar")
    if not os.path.isfile(wfn):
        torch.manual_seed(3)
        net = G.PoseNet(G.resnet34(_binding=emu), droprate=0.0, pretrained=False, _binding=emu)
        torch.save({"model_state_dict": net.state_dict()}, wfn)
    s = configparser.ConfigParser()
    s.read(os.path.join(ROOT, "scripts", "configs", config))
    s["hyperparameters"]["skip"], s["hyperparameters"]["steps"] = "2", str(steps)
    cfg = str(tmp_path / config)
    with open(cfg, "w") as f:
        s.write(f)
    argv = ["--model", "mapnet", "--config_file", cfg, "--weights", wfn, "--dtype", "fp32", "--synthetic_length", "3",
            "--height", str(H), "--width", str(W)]
    return eval_script, eval_script.build_parser().parse_args(argv + list(extra))


def _run(emu, tmp_path, tag, config, extra):
    script, args = _eval_args(tmp_path, emu, config, list(extra) + ["--sequence", "--batch_frames", "4", "--output_dir", str(tmp_path / tag)])
    lines = []
    summary, pred, targ = script.run(args, _binding=emu, log=lines.append)
    # the log lines and the .npz of a run without the flag (tests/test_emu_scripts.py)
    assert len(lines) == 4 and lines[0].startswith("Loaded weights from ") and lines[1] == "Running mapnet on TRAIN data"
    assert lines[2].startswith("Error in translation: median ") and "\nError in rotation: median " in lines[2]
    name = "Synthetic_synthetic_mapnet%s.npz" % ("_pgo" if "--pose_graph" in extra else "")
    assert lines[3] == "%s saved" % str(tmp_path / tag / name)
    z = np.load(str(tmp_path / tag / name))
    assert sorted(z.files) == sorted(["pred_poses", "targ_poses", "median_t", "mean_t", "median_q", "mean_q"])
    np.testing.assert_array_equal(z["pred_poses"], pred)
    np.testing.assert_array_equal(z["targ_poses"], targ)
    assert pred.shape == targ.shape == (3, 7) and np.isfinite(pred).all() and set(summary) == {"median_t", "mean_t", "median_q", "mean_q"}
    return summary, pred, targ


def test_eval_script_sequence(emu, tmp_path):
    """--sequence: three frames, one forward pass (the loop would run three); frames from a resident store: the same numbers"""
    from geomapnet_amd.data import SyntheticFrames
    import geomapnet_amd.evaluate as E
    _, pred, targ = _run(emu, tmp_path, "plain", "synthetic_mapnet.ini", ["--u8_input"])
    np.testing.assert_array_equal(targ, E.to_pose7(SyntheticFrames(3, H=8, W=8, seed=7).poses.numpy(), np.zeros(3), np.ones(3)))
    _, pred_r, targ_r = _run(emu, tmp_path, "resident", "synthetic_mapnet.ini", ["--u8_input", "--resident_frames"])
    assert np.array_equal(pred_r, pred) and np.array_equal(targ_r, targ)


def test_eval_script_sequence_pose_graph(emu, tmp_path):
    _, pred, _ = _run(emu, tmp_path, "pgo", "synthetic_pose_graph.ini", ["--pose_graph"])
    np.testing.assert_allclose(np.linalg.norm(pred[:, 3:], axis=1), 1.0, atol=1e-9)  # optimised poses carry unit quaternions


@pytest.mark.parametrize("extra", [["--batch_frames", "8"], ["--resident_frames"]], ids=["batch_frames", "resident_frames"])
def test_eval_script_flags_need_sequence(emu, tmp_path, extra):
    script, args = _eval_args(tmp_path, emu, "synthetic_mapnet.ini", extra)
    with pytest.raises(SystemExit, match="--sequence"):
        script.run(args, _binding=emu, log=lambda *a: None)


# ---- GPU suite ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,N,fc", K.OP_CASES, ids=_IDS)
def test_gpu_op_seq_windows(hip, W, N, fc):
    K.check_op_case(hip, "cuda", W, N, fc)


@pytest.mark.gpu
def test_gpu_op_seq_windows_clamped(hip):
    K.check_op_clamped(hip, "cuda")


@pytest.mark.gpu
def test_gpu_op_seq_windows_errors(hip):
    K.check_op_errors(hip, "cuda")


@pytest.mark.gpu
def test_gpu_optimize_windows_dev(hip):
    K.check_optimize_windows_dev(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name,form,fused", [("fp32", "fp32", False), ("fp32", "u8", False), ("fp16x2m", "fp32", True),
                                                   ("fp16x2m", "u8", True)],
                         ids=["fp32", "fp32-u8", "fp16x2m-fused", "fp16x2m-fused-u8"])
def test_gpu_pose_table(hip, dtype_name, form, fused):
    K.check_pose_table(hip, "cuda", dtype_name, form, fused)


@pytest.mark.gpu
def test_gpu_refusals(hip):
    K.check_refusals(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name,fused", [("fp32", False), ("fp16x2m", True)], ids=["fp32", "fp16x2m-fused"])
def test_gpu_against_loop(hip, dtype_name, fused):
    K.check_against_loop(hip, "cuda", dtype_name, fused)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name,fused", [("fp32", False), ("fp16x2m", True)], ids=["fp32", "fp16x2m-fused"])
@pytest.mark.parametrize("steps,fc", PGO_CASES, ids=_PGO_IDS)
def test_gpu_against_loop_pose_graph(hip, steps, fc, dtype_name, fused):
    K.check_against_loop_pose_graph(hip, "cuda", dtype_name, steps, fc, fused)
