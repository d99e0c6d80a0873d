"""Input gradient of the poses at inference (csrc/input_grad.h, mn_input_grad; the reference's scripts/plot_activations.py).  CPU
tests run the kernels in the SIMT emulator at small sizes; the GPU tests (-m gpu) run the same checks on libmapnet_hip.so."""
import os
import sys

import numpy as np
import pytest
import torch

import emu_lib
import input_grad_checks as IG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16 = 0, 1
# (B, H, W): every pixel near a border; even sizes (last row / column receive fewer taps); odd sizes over several tiles
STEM_SHAPES = [(2, 9, 11), (1, 32, 40), (3, 40, 53), (1, 33, 47)]


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


# ---- CPU suite (SIMT emulator) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_dgrad(emu, dtype, shape):
    IG.check_stem_dgrad(emu, "cpu", dtype, *shape)


@pytest.mark.parametrize("dtype", [F32, F16])
def test_bn_eval_bwd(emu, dtype):
    IG.check_bn_eval_bwd(emu, "cpu", dtype)


def test_saliency_op(emu):
    IG.check_saliency_op(emu, "cpu")


def test_input_grad_fp32(emu):
    IG.check_input_grad_vs_oracle(emu, "cpu", "fp32", N=1, T=3, H=40, W=53)  # (the MapNet wrapper's [N,T,...] path as well)


def test_input_grad_fp32_odd_size(emu):
    IG.check_input_grad_vs_oracle(emu, "cpu", "fp32", N=1, T=1, H=33, W=47)


def test_input_grad_fp32_cotangent(emu):
    IG.check_input_grad_vs_oracle(emu, "cpu", "fp32", N=1, T=2, H=40, W=53, cotangent=True)


def test_input_grad_fp16(emu):
    """measured (emulator, seed 7, (1,2,40,53), loss scale 1024): device 9.5e-2 / 1.27e-1 per image against the float64 oracle; the
    oracle itself with fp16 storage sits at 1.05e-1 / 1.16e-1 (random weights: fp16-rounded activations flip ReLU gates)"""
    IG.check_input_grad_vs_oracle(emu, "cpu", "fp16", N=1, T=2, H=40, W=53)


def test_input_grad_u8(emu):
    IG.check_u8_input(emu, "cpu")


def test_leaves_training_state(emu, monkeypatch):
    monkeypatch.setenv("MN_DETERMINISTIC", "1")
    IG.check_leaves_training_state(emu, "cpu", "fp32")


def test_leaves_training_state_fp16(emu, monkeypatch):
    monkeypatch.setenv("MN_DETERMINISTIC", "1")
    IG.check_leaves_training_state(emu, "cpu", "fp16")


def test_errors(emu):
    IG.check_errors(emu, "cpu")


# ---- host side -------------------------------------------------------------------------------------------------------------------
def test_attention_overlay_by_hand():
    from geomapnet_amd.evaluate import attention_overlay
    mean, std = (0.5, 0.25, 0.0), (0.5, 0.25, 1.0)
    amap = np.array([[0.0, 1.0], [0.5, 0.25]])
    # un-normalised RGB in [0, 1]: pixel (0,0) = (1, .5, .2), (0,1) = (0, 0, 0), (1,0) = (2, 0, 0) (clips), (1,1) = (.5, .25, 1)
    rgb = np.array([[[1.0, 0.5, 0.2], [0.0, 0.0, 0.0]], [[2.0, 0.0, 0.0], [0.5, 0.25, 1.0]]])
    frame = ((rgb - np.array(mean)) / np.array(std)).transpose(2, 0, 1).astype(np.float32)
    out = attention_overlay(frame, amap, mean, std)
    assert out.shape == (2, 2, 3) and out.dtype == np.uint8
    # jet(0) = (0, 0, .5), jet(1) = (.5, 0, 0); the colour triple is added, unflipped, to the BGR image (as the reference does)
    assert out[0, 0].tolist() == [int(0.5 * 0.2 * 255 + 0), int(0.5 * 0.5 * 255 + 0), int(0.5 * 255 + 0.5 * 127.5)]
    assert out[0, 1].tolist() == [int(0.5 * 127.5), 0, 0]
    j = __import__("matplotlib").colormaps["jet"](0.5)[:3]
    assert out[1, 0].tolist() == [int(0.5 * 255 * j[0]), int(0.5 * 255 * j[1]), min(255, int(255 + 0.5 * 255 * j[2]))]
    # a uint8 frame [H,W,3] gives the same picture as its normalised form
    u8 = np.array([[[255, 128, 51], [0, 0, 0]], [[255, 0, 0], [128, 64, 255]]], dtype=np.uint8)
    fr2 = ((u8 / 255.0 - np.array(mean)) / np.array(std)).transpose(2, 0, 1)
    assert np.abs(attention_overlay(u8, amap, mean, std).astype(int) - attention_overlay(fr2, amap, mean, std).astype(int)).max() <= 1
    with pytest.raises(ValueError):
        attention_overlay(u8, np.zeros((3, 2)), mean, std)


def test_plot_activations_script(emu, tmp_path):
    from PIL import Image
    import geomapnet_amd as G
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import plot_activations as script
    G.set_compute_dtype("fp32")
    torch.manual_seed(3)
    net = G.PoseNet(G.resnet34(_binding=emu), droprate=0.0, pretrained=False, _binding=emu)
    wfn = str(tmp_path / "posenet_weights.pth.tar")
    torch.save({"model_state_dict": net.state_dict()}, wfn)
    args = script.build_parser().parse_args(
        ["--config_file", os.path.join(ROOT, "scripts", "configs", "synthetic_posenet.ini"), "--weights", wfn, "--synthetic_length", "2",
         "--height", "32", "--width", "40", "--output_dir", str(tmp_path / "att"), "--val"])
    assert args.dtype == "fp32"
    lines = []
    files = script.run(args, _binding=emu, log=lines.append)
    assert [os.path.basename(f) for f in files] == ["Synthetic_synthetic_attention_posenet_%05d.png" % i for i in (0, 1)]
    for f in files:
        im = Image.open(f)
        assert im.size == (40, 32) and im.mode == "RGB"
        assert np.asarray(im).std() > 0
    assert "Visualizing VAL data" in lines and lines[-1] == "2 frames written to %s" % str(tmp_path / "att")


# ---- GPU suite -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("shape", STEM_SHAPES + [(2, 256, 341)])
def test_gpu_stem_dgrad(hip, dtype, shape):
    IG.check_stem_dgrad(hip, "cuda", dtype, *shape)


@pytest.mark.gpu
def test_gpu_bn_eval_bwd_and_saliency(hip):
    IG.check_bn_eval_bwd(hip, "cuda", F32)
    IG.check_bn_eval_bwd(hip, "cuda", F16)
    IG.check_saliency_op(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(N=1, T=3, H=40, W=53), dict(N=1, T=1, H=33, W=47), dict(N=1, T=2, H=64, W=85),
                                  dict(N=1, T=2, H=40, W=53, cotangent=True)])
def test_gpu_input_grad_fp32(hip, case):
    IG.check_input_grad_vs_oracle(hip, "cuda", "fp32", **case)


@pytest.mark.gpu
def test_gpu_input_grad_fp16(hip):
    IG.check_input_grad_vs_oracle(hip, "cuda", "fp16", N=1, T=2, H=40, W=53)


@pytest.mark.gpu
def test_gpu_input_grad_u8(hip):
    IG.check_u8_input(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "fp16"])
def test_gpu_leaves_training_state(hip, monkeypatch, dtype_name):
    monkeypatch.setenv("MN_DETERMINISTIC", "1")
    IG.check_leaves_training_state(hip, "cuda", dtype_name)


@pytest.mark.gpu
def test_gpu_errors(hip):
    IG.check_errors(hip, "cuda")
