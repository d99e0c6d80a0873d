"""The criteria's loss functions (t_loss_fn / q_loss_fn of common/criterion.py:34,55,112: L1, MSE, SmoothL1, Huber, QuaternionLoss) in
the fused criterion kernel: mn_op_criterion_fn, mn_set_loss_fn and the Python facade.  CPU tests run the kernels in the SIMT
emulator; the GPU tests (-m gpu) run the same checks on libmapnet_hip.so."""
import configparser
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

import emu_lib
import loss_fn_checks as LF
import loss_fn_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (mode, N, T).  N = 1: a single lane active; 5; 257: the window loop of the one 256-thread workgroup runs twice and the four waves
# reduce unequal shares.  Mode 1: T = 2, 3 and kMaxT = 8; modes 2 and 3: T = 2 and 4 (2T = 8 rows).
SHAPES = [(0, 1, 1), (0, 5, 1), (0, 257, 1), (1, 1, 2), (1, 5, 3), (1, 257, 3), (1, 5, 8), (2, 1, 2), (2, 5, 4), (2, 257, 2),
          (3, 1, 2), (3, 5, 4), (3, 257, 2)]
PIECEWISE = [LF.SMOOTH_L1, LF.HUBER]


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


# ---- the restatement is the reference's ---------------------------------------------------------------------------------------
def test_restatement_is_pinned_to_the_reference_classes():
    """tests/loss_fn_ref.py against common/criterion.py itself (its three criterion classes and QuaternionLoss, executed through
    oracle/ref_loader.py) in float64, for every kind of either argument and every mode: loss, d pred and d s"""
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    rc = ref_loader.load()
    classes = {0: rc.criterion.PoseNetCriterion, 1: rc.criterion.MapNetCriterion, 2: rc.MapNetOnlineCriterionPy3,
               3: rc.MapNetOnlineCriterionPy3}

    def ref_module(kind, param):
        return rc.criterion.QuaternionLoss() if kind == LF.QUATERNION else LF.module(kind, param)

    for mode, N, T in ((0, 5, 1), (1, 3, 3), (2, 3, 2), (3, 3, 2)):
        pred, targ = LF.inputs(mode, N, T, seed=3)
        for tk in LF.T_KINDS:
            for qk in LF.Q_KINDS:
                kw = dict(sax=LF.S4[0], saq=LF.S4[1], learn_beta=True)
                if mode:
                    kw.update(srx=LF.S4[2], srq=LF.S4[3], learn_gamma=True)
                if mode >= 2:
                    kw["gps_mode"] = mode == 3
                theirs = classes[mode](t_loss_fn=ref_module(tk, 0.4), q_loss_fn=ref_module(qk, 0.2), **kw).double()
                p = pred.double().requires_grad_(True)
                loss = theirs(p, targ.double())
                loss.backward()
                wl, wdp, wds = LF.reference(mode, pred, targ, LF.S4, LF.module(tk, 0.4), LF.module(qk, 0.2))
                assert abs(loss.item() - wl) < 1e-12, (mode, tk, qk)
                np.testing.assert_allclose(p.grad.numpy(), wdp.numpy(), rtol=0, atol=1e-12)
                names = ("sax", "saq") if mode == 0 else ("sax", "saq", "srx") if mode == 3 else ("sax", "saq", "srx", "srq")
                for n, w in zip(names, wds):
                    assert abs(getattr(theirs, n).grad.item() - w) < 1e-12, (mode, tk, qk, n)


# ---- CPU suite (SIMT emulator) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_every_pair_of_kinds(emu, shape):
    LF.check_pairs(emu, "cpu", *shape)


@pytest.mark.parametrize("kind", PIECEWISE)
def test_hand_built_breakpoints(emu, kind):
    LF.check_hand_built(emu, "cpu", kind)


def test_default_op_unchanged(emu, golden_dir):
    LF.check_default_op_unchanged(emu, "cpu", golden_dir)


def test_default_plan_unchanged(emu, monkeypatch):
    monkeypatch.setenv("MN_DETERMINISTIC", "1")
    LF.check_default_plan_unchanged(emu, "cpu", "fp32")


@pytest.mark.parametrize("dtype_name", ["fp32", "fp16x2m"])
def test_fused_step_mse_smooth_l1(emu, dtype_name):
    LF.check_fused_step(emu, "cpu", dtype_name)


def test_facade(emu):
    LF.check_facade(emu, "cpu")


def test_train_script_with_loss_functions(emu, tmp_path):
    """scripts/train.py --t_loss_fn mse --q_loss_fn quaternion: two steps on synthetic frames, a finite logged loss; the validation
    criterion stays L1"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train as train_script
    s = configparser.ConfigParser()
    s.read(os.path.join(ROOT, "scripts", "configs", "synthetic_mapnet.ini"))
    s["training"].update(n_epochs="1", batch_size="2", snapshot="1", do_val="no", val_freq="1")
    s["hyperparameters"]["skip"] = "1"
    s["logging"]["print_freq"] = "1"
    cfg = str(tmp_path / "synthetic_mapnet.ini")
    with open(cfg, "w") as f:
        s.write(f)
    args = train_script.build_parser().parse_args(
        ["--model", "mapnet", "--config_file", cfg, "--dtype", "fp32", "--synthetic_length", "4", "--synthetic_val_length",
         "1", "--height", "32", "--width", "40", "--logdir", str(tmp_path / "logs"), "--num_workers", "0", "--learn_beta",
         "--learn_gamma", "--t_loss_fn", "mse", "--q_loss_fn", "quaternion"])
    assert args.loss_param == 1.0
    assert train_script.build_parser().parse_args(["--model", "mapnet"]).t_loss_fn == "l1"
    lines = []
    tr = train_script.run(args, _binding=emu, log=lines.append)
    assert isinstance(tr.train_criterion.t_loss_fn, nn.MSELoss) and type(tr.train_criterion.q_loss_fn).__name__ == "QuaternionLoss"
    assert isinstance(tr.val_criterion.t_loss_fn, nn.L1Loss) and isinstance(tr.val_criterion.q_loss_fn, nn.L1Loss)
    train_lines = [l for l in lines if l.startswith("Train ")]
    assert len(train_lines) == 2, lines
    eng = tr.model.mapnet._engine
    assert [p["loss_fn"] for p in eng.plans.values() if "loss_fn" in p] == [(LF.MSE, 0.0, LF.QUATERNION, 0.0)]
    for l in train_lines:
        assert np.isfinite(float(l.split("Loss ")[1].split()[0])), l
    with pytest.raises(NotImplementedError):
        bad = train_script.build_parser().parse_args(["--model", "mapnet", "--config_file", cfg, "--t_loss_fn", "quaternion"])
        train_script.run(bad, _binding=emu, log=lambda *a: None)


# ---- GPU suite ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_every_pair_of_kinds(hip, shape):
    LF.check_pairs(hip, "cuda", *shape)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PIECEWISE)
def test_gpu_hand_built_breakpoints(hip, kind):
    LF.check_hand_built(hip, "cuda", kind)


@pytest.mark.gpu
def test_gpu_default_op_unchanged(hip, golden_dir):
    LF.check_default_op_unchanged(hip, "cuda", golden_dir)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "fp16x2m"])
def test_gpu_default_plan_unchanged(hip, monkeypatch, dtype_name):
    monkeypatch.setenv("MN_DETERMINISTIC", "1")
    LF.check_default_plan_unchanged(hip, "cuda", dtype_name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "fp16x2m"])
def test_gpu_fused_step_mse_smooth_l1(hip, dtype_name):
    LF.check_fused_step(hip, "cuda", dtype_name)


@pytest.mark.gpu
def test_gpu_facade(hip):
    LF.check_facade(hip, "cuda")
