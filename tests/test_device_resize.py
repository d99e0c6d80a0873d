"""Resize on the device for uint8 input (csrc/resize.h, mn_set_input_resize): torchvision's Resize = PIL's bilinear resample, bit for
bit.  tests/resize_ref.py restates Pillow's algorithm and is pinned to the installed Pillow here; the kernel and every plan-level
call are held to it exactly.  CPU tests run the kernels in the SIMT emulator at small sizes; the GPU tests (-m gpu) run them on
libmapnet_hip.so, at the real frame sizes too."""
import configparser
import os
import sys

import numpy as np
import pytest
import torch

import emu_lib
import resize_checks as RC
import resize_ref as R
from geomapnet_amd.data import resize_dims

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


# ---- the yardstick: resize_ref = Pillow -----------------------------------------------------------------------------------------
PILLOW_CASES = [(480, 640, 256), (960, 1280, 256), (37, 53, 16), (53, 37, 16), (20, 31, 32), (64, 64, 24), (48, 64, 48), (9, 200, 7),
                (48, 64, (48, 40))]


@pytest.mark.parametrize("h,w,size", PILLOW_CASES)
@pytest.mark.parametrize("binary", [False, True], ids=["noise", "0-255"])
def test_ref_equals_pillow(h, w, size, binary):
    from PIL import Image
    H, W = resize_dims(h, w, size)
    f = RC.frames(1, h, w, seed=h + w, binary=binary)[0].numpy()
    want = np.asarray(Image.fromarray(f).resize((W, H), Image.BILINEAR))
    assert np.array_equal(R.resize(f, H, W), want)


def test_resize_dims():
    assert resize_dims(480, 640, 256) == (256, 341)
    assert resize_dims(640, 480, 256) == (341, 256)
    assert resize_dims(960, 1280, 256) == (256, 341)
    assert resize_dims(64, 64, 24) == (24, 24)
    assert resize_dims(48, 64, (48, 40)) == (48, 40)
    assert resize_dims(9, 200, 7) == (7, 155)


# ---- CPU suite (SIMT emulator) -------------------------------------------------------------------------------------------------
def test_op_ragged_shapes(emu):
    RC.check_op_shapes(emu, "cpu")


def test_op_three_by_three_tiles(emu):
    RC.check_multi_tile(emu, "cpu")  # 75x300 -> 40x160 in tiles of 16 rows x 64 columns


def test_plan_forward(emu):
    RC.check_forward(emu, "cpu", "fp32", B=3, src=(48, 64), size=32)


def test_plan_forward_with_jitter(emu):
    RC.check_forward(emu, "cpu", "fp32", B=3, src=(48, 64), size=32, jitter=True)


def test_plan_train_step(emu):
    RC.check_train_step(emu, "cpu", "fp32", N=1, T=2, src=(48, 64), size=32)


def test_plan_train_step_with_jitter(emu):
    RC.check_train_step(emu, "cpu", "fp32", N=1, T=2, src=(48, 64), size=32, jitter=True)


def test_plan_input_gradient_and_saliency(emu):
    RC.check_input_grad(emu, "cpu", "fp32", B=2, src=(48, 64), size=32)


def test_off_is_off(emu):
    RC.check_off_is_off(emu, "cpu")


def test_errors(emu):
    RC.check_errors(emu, "cpu")


def _script_args(module, tmp_path, extra):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    mod = __import__(module)
    s = configparser.ConfigParser()
    s.read(os.path.join(ROOT, "scripts", "configs", "synthetic_mapnet.ini"))
    s["training"].update(n_epochs="1", batch_size="2", snapshot="1", val_freq="1", do_val="yes")
    s["hyperparameters"]["skip"] = "1"
    cfg = str(tmp_path / "synthetic_mapnet.ini")
    with open(cfg, "w") as f:
        s.write(f)
    argv = ["--model", "mapnet", "--config_file", cfg, "--dtype", "fp32", "--synthetic_length", "2", "--synthetic_val_length", "1",
            "--height", "48", "--width", "64", "--logdir", str(tmp_path / "logs"), "--num_workers", "0"]
    return mod, mod.build_parser().parse_args(argv + list(extra))


def test_train_script_flag(emu, tmp_path):
    train_script, args = _script_args("train", tmp_path, ["--u8_input", "--device_resize", "32"])
    tr = train_script.run(args, _binding=emu, log=lambda *a: None)
    eng = RC.engine(tr.model)
    assert eng.input_resize == 32
    plans = list(eng.plans.values())
    assert plans and all(p["src"] == (48, 64) and (p["cfg"].H, p["cfg"].W) == (32, 42) for p in plans)
    assert np.isfinite(tr.last_val_loss)
    train_script, args = _script_args("train", tmp_path, ["--device_resize", "32"])
    with pytest.raises(SystemExit, match="--u8_input"):
        train_script.run(args, _binding=emu, log=lambda *a: None)


@pytest.mark.parametrize("script", ["eval", "plot_activations"])
def test_other_scripts_need_u8_input(script, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    mod = __import__(script)
    args = mod.build_parser().parse_args(["--dataset", "Synthetic", "--scene", "s", "--weights", "none.pth.tar", "--device_resize", "32"]
                                        + (["--output_dir", str(tmp_path)] if script == "plot_activations" else []))
    with pytest.raises(SystemExit, match="--u8_input"):
        mod.run(args)


# ---- GPU suite ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_op_ragged_shapes(hip):
    RC.check_op_shapes(hip, "cuda")
    RC.check_multi_tile(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("sh,sw,H,W", [(480, 640, 256, 341), (960, 1280, 256, 341), (640, 480, 341, 256)])
def test_gpu_op_real_frames(hip, sh, sw, H, W):
    assert resize_dims(sh, sw, 256) == (H, W)
    RC.check_op(hip, "cuda", 2, sh, sw, H, W, seed=70)


@pytest.mark.gpu
def test_gpu_plan_fp16x2m_forward_and_train_step(hip):
    RC.check_forward(hip, "cuda", "fp16x2m", B=2, src=(120, 160), size=64)
    RC.check_train_step(hip, "cuda", "fp16x2m", N=1, T=2, src=(120, 160), size=64, jitter=True)


@pytest.mark.gpu
def test_gpu_plan_fp32_input_gradient_and_saliency(hip):
    RC.check_input_grad(hip, "cuda", "fp32", B=2, src=(75, 100), size=40)


@pytest.mark.gpu
def test_gpu_off_is_off_and_errors(hip):
    RC.check_off_is_off(hip, "cuda")
    RC.check_errors(hip, "cuda")
