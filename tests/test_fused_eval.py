"""The fused inference pass (mn_set_eval_fused, mn_op_conv_bn_eval; csrc/igemm.h Epilogue::bn_coef): BatchNorm, residual and ReLU in
the epilogues of the h2 forward convolutions.  CPU tests run the kernels in the SIMT emulator at small sizes; the GPU tests (-m gpu)
run the same checks on libmapnet_hip.so.  Layer1 ships on the fused instantiation of conv_halo_h2_kernel (no scratch), so the
plan-level bit equality covers it."""
import os
import subprocess
import sys

import pytest
import torch

import emu_lib
import fused_eval_checks as FE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEFAULT_SHAPES = FE.HALO_H2_SHAPES + FE.IGEMM_SHAPES + FE.IGEMM64_SHAPES + FE.HALO64_SHAPES + FE.HALO480_SHAPES


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


def run_forced(backend, group):
    knob, value, _ = __import__("fused_eval_cases").GROUPS[group]
    env = dict(os.environ, FUSED_EVAL_GROUP=group, **{knob: value})
    subprocess.run([sys.executable, os.path.join(HERE, "fused_eval_cases.py"), backend], check=True, env=env, timeout=300)


# ---- CPU suite (SIMT emulator) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DEFAULT_SHAPES)
def test_op(emu, shape):
    FE.check_op(emu, "cpu", shape, log=print)


@pytest.mark.parametrize("group", ["a1", "halo256"])
def test_op_forced_shapes(group):
    run_forced("emu", group)


def test_op_refusals(emu):
    FE.check_op_refusals(emu, "cpu")


def test_refusals(emu):
    FE.check_refusals(emu, "cpu")


@pytest.mark.parametrize("dtype_name,mapnet", [("fp16x2m", False), ("fp16x2", True)])
def test_plan_against_unfused(emu, dtype_name, mapnet):
    """poses and activations equal where the host build gives equality (it does with the compiler this was written on); where it
    does not, the poses agree to a few fp32 ulps of the pose scale and the figure is printed.  The fused pass leaves the raw conv
    outputs unwritten; turning the switch off again reproduces the first pass."""
    diff = FE.check_plan_bit_equal(emu, "cpu", dtype_name, mapnet, 64, 85, require=False)
    print("largest pose difference fused - unfused (emulator, %s): %.3e" % (dtype_name, diff))


def test_eval_forward_against_oracle(emu):
    FE.check_eval_forward_fused(emu, "cpu", "fp16x2m", B=3, H=64, W=85)


def test_coefficients_never_stale(emu):
    FE.check_coefficients_never_stale(emu, "cpu", H=32, W=40, require=False)


# ---- GPU suite -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", DEFAULT_SHAPES + FE.HALO384_SHAPES)
def test_gpu_op(hip, shape):
    FE.check_op(hip, "cuda", shape, log=print)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["a1", "halo256"])
def test_gpu_op_forced_shapes(group):
    run_forced("hip", group)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FE.RACE_SHAPES)
def test_gpu_op_many_workgroups(hip, shape):
    FE.check_op(hip, "cuda", shape, variants=((True, True),), log=print)


@pytest.mark.gpu
def test_gpu_op_refusals(hip):
    FE.check_op_refusals(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["fp16x2m", "fp16x2"])
@pytest.mark.parametrize("mapnet,H,W", [(False, 128, 171), (True, 64, 85)])
def test_gpu_plan_bit_equal(hip, dtype_name, mapnet, H, W):
    FE.check_plan_bit_equal(hip, "cuda", dtype_name, mapnet, H, W)


@pytest.mark.gpu
def test_gpu_eval_forward_against_oracle(hip):
    FE.check_eval_forward_fused(hip, "cuda", "fp16x2m", B=3, H=128, W=171)


@pytest.mark.gpu
def test_gpu_coefficients_never_stale(hip):
    FE.check_coefficients_never_stale(hip, "cuda")


@pytest.mark.gpu
def test_gpu_training_state_untouched(hip, monkeypatch):
    monkeypatch.setenv("MN_DETERMINISTIC", "1")
    FE.check_training_state_untouched(hip, "cuda")


@pytest.mark.gpu
def test_gpu_with_input_pipeline(hip):
    FE.check_with_input_pipeline(hip, "cuda")


@pytest.mark.gpu
def test_gpu_command_lines(hip, tmp_path):
    FE.check_command_lines(hip, tmp_path)
