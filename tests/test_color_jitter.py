"""ColorJitter on the device for uint8 input (csrc/jitter.h, mn_set_color_jitter): torchvision's ColorJitter on x = u8 / 255 before
Normalize, against the float64 restatement of tests/jitter_ref.py.  CPU tests run the kernels in the SIMT emulator at small
sizes; the GPU tests (-m gpu) run them on libmapnet_hip.so at BASELINE's full size."""
import configparser
import os
import sys

import numpy as np
import pytest
import torch

import checks
import emu_lib
import jitter_checks as J
import jitter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---- the restatement itself: hand-checked cases ----------------------------------------------------------------------------------
def test_ref_gray_pixel_unchanged_by_hue():
    x = np.full((2, 3, 3), 0.4)
    for h in (-0.5, -0.2, 0.1, 0.5):
        assert np.allclose(R.adjust_hue(x, h), x, atol=1e-12)


def test_ref_red_plus_third_is_green():
    red = np.array([[[1.0, 0.0, 0.0]]])
    assert np.allclose(R.adjust_hue(red, 1.0 / 3.0), [[[0.0, 1.0, 0.0]]], atol=1e-12)
    assert np.allclose(R.adjust_hue(red, -1.0 / 3.0), [[[0.0, 0.0, 1.0]]], atol=1e-12)


def test_ref_contrast_zero_is_mean_gray():
    x = np.random.default_rng(0).random((5, 7, 3))
    m = (0.2989 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]).mean()
    assert np.allclose(R.adjust_contrast(x, 0.0), m, atol=1e-12)


def test_ref_hsv_round_trip_and_saturation_zero_is_gray():
    x = np.random.default_rng(1).random((6, 9, 3))
    assert np.allclose(R.hsv2rgb(R.rgb2hsv(x)), x, atol=1e-12)
    g = R.adjust_saturation(x, 0.0)
    assert np.allclose(g, R.gray(x)[..., None], atol=1e-12)
    assert np.allclose(R.adjust_brightness(x, 3.0), np.clip(3.0 * x, 0, 1))


# ---- CPU suite (SIMT emulator) -------------------------------------------------------------------------------------------------
def test_each_op_alone(emu):
    J.check_single_ops(emu, "cpu", B=6, H=40, W=53)


def test_all_ops_plan_pass(emu):
    J.check_all_ops(emu, "cpu", B=6, H=40, W=53, all_orders=False)


def test_all_24_orders(emu):
    J.check_op_orders(emu, "cpu")


def test_draw_statistics(emu):
    J.check_draws(emu, "cpu", images=4096)


def test_pass_sequence_across_plans(emu):
    J.check_sequence(emu, "cpu")


def test_off_is_off(emu):
    J.check_off_is_off(emu, "cpu")


def test_train_step_matches_oracle(emu):
    J.check_train_step(emu, "cpu", "fp32", N=2, T=3, H=64, W=85)


def test_errors(emu):
    J.check_errors(emu, "cpu")


def test_checkpoint_carries_pass_count(emu):
    import geomapnet_amd as G
    from geomapnet_amd.train import load_checkpoint, save_checkpoint
    net = J.model(emu, "cpu", mapnet=True)
    c = G.MapNetCriterion(_binding=emu)
    opt = G.Optimizer([{"params": net.parameters()}], "adam", base_lr=1e-4, weight_decay=0.0)
    assert "color_jitter_calls" not in save_checkpoint(None, 0, net, opt, c)  # jitter off: the reference's dict
    net.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=4)
    J.engine(net).set_color_jitter_calls(17)
    ck = save_checkpoint(None, 3, net, opt, c)
    assert ck["color_jitter_calls"] == 17
    other = J.model(emu, "cpu", mapnet=True)
    other.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=4)
    opt2 = G.Optimizer([{"params": other.parameters()}], "adam", base_lr=1e-4, weight_decay=0.0)
    load_checkpoint(ck, other, opt2, G.MapNetCriterion(_binding=emu), resume_optim=True)
    assert J.engine(other).jitter_calls == 17


def _train_args(tmp_path, extra):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train as train_script
    s = configparser.ConfigParser()
    s.read(os.path.join(ROOT, "scripts", "configs", "synthetic_mapnet.ini"))
    s["training"].update(n_epochs="1", batch_size="2", snapshot="1", val_freq="1", do_val="yes")
    s["hyperparameters"]["skip"] = "1"
    cfg = str(tmp_path / "synthetic_mapnet.ini")
    with open(cfg, "w") as f:
        s.write(f)
    argv = ["--model", "mapnet", "--config_file", cfg, "--dtype", "fp32", "--synthetic_length", "2", "--synthetic_val_length", "1",
            "--height", "32", "--width", "40", "--logdir", str(tmp_path / "logs"), "--num_workers", "0"]
    return train_script, train_script.build_parser().parse_args(argv + list(extra))


def test_train_script_flag(emu, tmp_path):
    train_script, args = _train_args(tmp_path, ["--u8_input", "--device_color_jitter"])
    lines = []
    tr = train_script.run(args, _binding=emu, log=lines.append)
    assert "Using ColorJitter data augmentation" in lines
    eng = J.engine(tr.model)
    assert eng.color_jitter[:4] == (0.7, 0.7, 0.7, 0.5)
    assert eng.jitter_calls >= 2  # the training batch and the validation batches
    assert np.isfinite(tr.last_val_loss)
    train_script, args = _train_args(tmp_path, ["--device_color_jitter"])
    with pytest.raises(SystemExit, match="--u8_input"):
        train_script.run(args, _binding=emu, log=lambda *a: None)


def test_train_script_without_flag_keeps_jitter_off(emu, tmp_path):
    train_script, args = _train_args(tmp_path, ["--u8_input"])
    lines = []
    tr = train_script.run(args, _binding=emu, log=lines.append)
    assert "Using ColorJitter data augmentation" not in lines
    eng = J.engine(tr.model)
    assert not eng.jitter_active() and eng.jitter_calls == 0


# ---- GPU suite ------------------------------------------------------------------------------------------------------------------
B_FULL, H_FULL, W_FULL = 192, 256, 341


@pytest.mark.gpu
def test_gpu_each_op_alone_full_size(hip):
    J.check_single_ops(hip, "cuda", B=B_FULL, H=H_FULL, W=W_FULL)


@pytest.mark.gpu
def test_gpu_all_orders_full_size(hip):
    J.check_all_ops(hip, "cuda", B=B_FULL, H=H_FULL, W=W_FULL, max_passes=4)


@pytest.mark.gpu
def test_gpu_off_is_off_full_size(hip):
    J.check_off_is_off(hip, "cuda", B=B_FULL, H=H_FULL, W=W_FULL)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp16x2m", "fp16"])
def test_gpu_fp16_modes_single_and_all_ops(hip, dtype):
    # fp16x2m keeps the input in fp32 (the fp16 copy for its stem backward kernels comes from the same values); fp16 stores it as
    # fp16: rel is that storage rounding
    J.check_single_ops(hip, "cuda", dtype, B=B_FULL, H=H_FULL, W=W_FULL, rel=2.0 ** -11)
    J.check_all_ops(hip, "cuda", dtype, B=B_FULL, H=H_FULL, W=W_FULL, max_passes=4, rel=2.0 ** -11)


@pytest.mark.gpu
def test_gpu_draws_and_sequence(hip):
    J.check_draws(hip, "cuda", images=1 << 16)
    J.check_op_orders(hip, "cuda", B=192, H=64, W=85)
    J.check_sequence(hip, "cuda", B=B_FULL, H=H_FULL, W=W_FULL)
    J.check_errors(hip, "cuda")


@pytest.mark.gpu
def test_gpu_train_step_matches_oracle(hip):
    J.check_train_step(hip, "cuda", "fp32", N=8, T=3, H=H_FULL, W=W_FULL)


@pytest.mark.gpu
def test_gpu_device_feed_u8_jitter_is_reproducible(hip):
    import geomapnet_amd as G
    G.set_compute_dtype("fp16x2m")
    gen = torch.Generator().manual_seed(3)
    N, T = 8, 3
    xs = [torch.randint(0, 256, (N, T, H_FULL, W_FULL, 3), generator=gen, dtype=torch.uint8).pin_memory() for _ in range(4)]
    ts = [(torch.randn(N, T, 6, generator=gen) * 0.3).pin_memory() for _ in range(4)]

    def run():
        old = os.environ.get("MN_DETERMINISTIC")
        os.environ["MN_DETERMINISTIC"] = "1"
        try:
            _, net = checks.build_pair(hip, "cuda")
            net.set_input_u8(J.MEAN, J.STD)
            net.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=9)
            c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=hip)
            opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                              base_lr=1e-4, weight_decay=5e-4)
            net.train()
            losses = [float(G.step_feedfwd(x, net, True, t, c, opt, True)[0]) for x, t in G.DeviceFeed(list(zip(xs, ts)), "cuda")]
            assert J.engine(net).jitter_calls == 4
            return losses
        finally:
            os.environ.pop("MN_DETERMINISTIC", None)
            if old is not None:
                os.environ["MN_DETERMINISTIC"] = old

    a, b = run(), run()
    assert all(np.isfinite(a)) and a == b, (a, b)
