"""Dataset pixel statistics on the device (csrc/frame_stats.h, mn_op_frame_stats_u8, geomapnet_amd/stats.py, scripts/dataset_mean.py,
--stats_file / --stats_from_frames): sums of bytes are integers, so the kernel and `pixel_sums` are held to numpy's int64 sums exactly;
mean and variance are held to the reference's float arithmetic within its own rounding.  CPU tests run the kernels in the SIMT
emulator; the GPU tests (-m gpu) run the same checks on libmapnet_hip.so, plus 192 saturated frames of 256x341 through one workgroup."""
import configparser
import os
import sys

import numpy as np
import pytest
import torch

import emu_lib
import frame_stats_checks as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 33, 47


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


# ---- CPU suite (SIMT emulator): the operator --------------------------------------------------------------------------------------
def test_op_shapes_and_alignments(emu):
    FC.check_shapes(emu, "cpu")


def test_op_indexed(emu):
    FC.check_indexed(emu, "cpu")


def test_op_accumulate(emu):
    FC.check_accumulate(emu, "cpu")


def test_op_blocks(emu):
    FC.check_blocks(emu, "cpu")


def test_op_saturated_frames(emu):
    FC.check_saturated(emu, "cpu")


# ONE saturated frame of 4400 x 4000 (52.8 MB, 4 297 units) through ONE workgroup: each of its 256 lanes sees 68 750 bytes of 255 per
# channel, more than the 66 051 a 32-bit accumulator holds, and the frame crosses the kernel's widening step (every 4 096 units)
WIDEN_CASE = (1, 4400, 4000)


def test_op_lane_accumulators_are_widened_in_time(emu):
    FC.check_saturated(emu, "cpu", *WIDEN_CASE, blocks=1)


def test_op_errors(emu):
    FC.check_errors(emu, "cpu")


# ---- geomapnet_amd.stats -----------------------------------------------------------------------------------------------------------
def test_pixel_sums_sources_chunks_and_add(emu):
    FC.check_sources(emu, "cpu")


def test_pixel_sums_after_resize(emu):
    FC.check_resize(emu, "cpu")


def test_against_the_reference_arithmetic(emu):
    FC.check_against_reference(emu, "cpu")


def test_reference_restatement_has_the_budgeted_roundings():
    """the bound's premise, on the host alone: the reference's arithmetic stays within the counted roundings of the exact integers"""
    from geomapnet_amd.stats import PixelSums
    u8 = FC.frames(20, 12, 17, seed=220)
    s = FC.np_sums(u8)
    exact = PixelSums(20 * 12 * 17, s[:3], s[3:])
    rm, rv = FC.reference_stats(u8)
    assert np.abs(exact.mean() - rm).max() <= FC.MEAN_BOUND and np.abs(exact.var() - rv).max() <= FC.VAR_BOUND


def test_write_and_read_stats(tmp_path):
    from geomapnet_amd import PixelSums, read_stats, write_stats
    u8 = FC.frames(4, 9, 11, seed=230)
    s = FC.np_sums(u8)
    sums = PixelSums(4 * 9 * 11, s[:3], s[3:])
    path = str(tmp_path / "stats.txt")
    assert write_stats(path, sums) == path
    want = str(tmp_path / "want.txt")
    np.savetxt(want, np.vstack((sums.mean(), sums.var())), fmt="%8.7f")
    with open(path, "rb") as a, open(want, "rb") as b:
        assert a.read() == b.read()
    rows = np.loadtxt(path)
    mean, std = read_stats(path)
    assert np.array_equal(mean, rows[0]) and np.array_equal(std, np.sqrt(rows[1]))  # the second row is the variance
    assert np.allclose(mean, sums.mean(), rtol=0, atol=5.1e-8) and np.allclose(std ** 2, sums.var(), rtol=0, atol=5.1e-8)
    write_stats(path, sums + PixelSums(0, [0, 0, 0], [0, 0, 0]))  # merging nothing: the same file
    with open(path, "rb") as a, open(want, "rb") as b:
        assert a.read() == b.read()


# ---- scripts (emulator) ------------------------------------------------------------------------------------------------------------
def _scripts():
    p = os.path.join(ROOT, "scripts")
    if p not in sys.path:
        sys.path.insert(0, p)


def _train_args(tmp_path, extra, name="run", dtype="fp32"):
    _scripts()
    import train as train_script
    s = configparser.ConfigParser()
    s.read(os.path.join(ROOT, "scripts", "configs", "synthetic_posenet.ini"))
    s["training"].update(n_epochs="0", batch_size="2", snapshot="1", val_freq="1")  # construction only: the weights stay the seed's
    cfg = str(tmp_path / "synthetic_posenet.ini")
    with open(cfg, "w") as f:
        s.write(f)
    argv = ["--model", "posenet", "--config_file", cfg, "--dtype", dtype, "--synthetic_length", "3", "--synthetic_val_length", "1",
            "--height", str(H), "--width", str(W), "--logdir", str(tmp_path / ("logs_" + name)), "--num_workers", "0"]
    return train_script, train_script.build_parser().parse_args(argv + list(extra)), s.getint("training", "seed")


def test_dataset_mean_script(emu, tmp_path):
    _scripts()
    import dataset_mean
    from geomapnet_amd import pixel_sums, read_stats
    from geomapnet_amd.data import SyntheticFrames
    out = str(tmp_path / "sub" / "stats.txt")
    args = dataset_mean.build_parser().parse_args(["--dataset", "Synthetic", "--scene", "s", "--synthetic_length", "5", "--height",
                                                   str(H), "--width", str(W), "--seed", "11", "--batch_frames", "2", "--output", out])
    lines = []
    assert dataset_mean.run(args, _binding=emu, log=lines.append) == out
    assert lines[0].startswith("Mean pixel = ") and lines[1].startswith("Std. pixel = ") and lines[2] == out + " written"
    frames = SyntheticFrames(5, H=H, W=W, seed=11, uint8=True)
    sums = pixel_sums(frames, _binding=emu)
    x = torch.stack([frames[i][0] for i in range(5)])
    assert FC.same(sums, FC.expect(x))
    want = str(tmp_path / "want.txt")
    np.savetxt(want, np.vstack((sums.mean(), sums.var())), fmt="%8.7f")
    assert np.array_equal(np.loadtxt(out), np.loadtxt(want))
    mean, std = read_stats(out)
    assert np.allclose(std, sums.std(), rtol=0, atol=1e-6)


def test_dataset_mean_refuses_real_datasets(emu):
    _scripts()
    import dataset_mean
    args = dataset_mean.build_parser().parse_args(["--dataset", "7Scenes", "--scene", "chess"])
    with pytest.raises(NotImplementedError):
        dataset_mean.run(args, _binding=emu, log=lambda *a: None)


def test_train_script_stats_file(emu, tmp_path):
    from geomapnet_amd import PixelSums, read_stats, write_stats
    import resize_checks as RC
    dark = FC.frames(2, 8, 8, seed=240, lo=0, hi=64)
    s = FC.np_sums(dark)
    path = write_stats(str(tmp_path / "stats.txt"), PixelSums(2 * 8 * 8, s[:3], s[3:]))
    mean, std = read_stats(path)
    quiet = lambda *a: None  # noqa: E731
    train_script, args, _ = _train_args(tmp_path, ["--u8_input", "--stats_file", path], "file", "fp16")
    with_file = train_script.run(args, _binding=emu, log=quiet).model
    _, args, _ = _train_args(tmp_path, ["--u8_input"], "plain", "fp16")  # (fp16: the emulator's quickest pass)
    plain = train_script.run(args, _binding=emu, log=quiet).model
    by_hand = train_script.run(args, _binding=emu, log=quiet).model  # the same seed: the same weights in all three
    by_hand.set_input_u8(mean, std)
    eng = RC.engine(with_file)
    assert eng.input_u8 == (tuple(float(v) for v in mean), tuple(float(v) for v in std))
    u8 = FC.frames(1, H, W, seed=241)
    pa, pb, pc = (RC.forward(m, u8) for m in (with_file, by_hand, plain))
    assert torch.isfinite(pa).all()
    assert torch.equal(pa, pb)  # bit for bit: the constants of the file, as set_input_u8 takes them by hand
    assert not torch.equal(pa, pc)  # and not the synthetic set's


def test_train_script_stats_from_frames(emu, tmp_path):
    _scripts()
    import dataset_mean
    import resize_checks as RC
    from geomapnet_amd import read_stats
    lines = []
    train_script, args, seed = _train_args(tmp_path, ["--u8_input", "--device_resize", "20", "--stats_from_frames"], "frames")
    tr = train_script.run(args, _binding=emu, log=lines.append)
    got = os.path.join(tr.logdir, "stats.txt")
    assert os.path.isfile(got)
    assert any(l.startswith("Mean pixel = ") for l in lines) and any(l.startswith("Std. pixel = ") for l in lines)
    out = str(tmp_path / "stats_dm.txt")
    dargs = dataset_mean.build_parser().parse_args(["--synthetic_length", "3", "--height", str(H), "--width", str(W), "--seed", str(seed),
                                                    "--device_resize", "20", "--output", out])
    dataset_mean.run(dargs, _binding=emu, log=lambda *a: None)
    with open(got, "rb") as a, open(out, "rb") as b:
        assert a.read() == b.read()
    # the model uses what it computed (unrounded), and they are the statistics of the RESIZED training frames
    from geomapnet_amd import pixel_sums
    from geomapnet_amd.data import SyntheticFrames
    sums = pixel_sums(SyntheticFrames(3, H=H, W=W, seed=seed, uint8=True), resize=20, _binding=emu)
    assert sums.count == 3 * 20 * 28
    assert RC.engine(tr.model).input_u8 == (tuple(sums.mean().tolist()), tuple(sums.std().tolist()))
    assert np.allclose(read_stats(got)[0], sums.mean(), rtol=0, atol=5.1e-8)


def test_flag_errors(emu, tmp_path):
    train_script, args, _ = _train_args(tmp_path, ["--stats_file", str(tmp_path / "none.txt")])
    with pytest.raises(SystemExit, match="--u8_input"):
        train_script.run(args, _binding=emu, log=lambda *a: None)
    _, args, _ = _train_args(tmp_path, ["--stats_from_frames"])
    with pytest.raises(SystemExit, match="--u8_input"):
        train_script.run(args, _binding=emu, log=lambda *a: None)
    _, args, _ = _train_args(tmp_path, ["--u8_input", "--stats_from_frames", "--stats_file", str(tmp_path / "none.txt")])
    with pytest.raises(SystemExit, match="exclude"):
        train_script.run(args, _binding=emu, log=lambda *a: None)


@pytest.mark.parametrize("script", ["eval", "plot_activations"])
def test_other_scripts_stats_file_needs_u8_input(script, tmp_path):
    _scripts()
    mod = __import__(script)
    args = mod.build_parser().parse_args(["--dataset", "Synthetic", "--scene", "s", "--weights", "none.pth.tar", "--stats_file", "s.txt"]
                                        + (["--output_dir", str(tmp_path)] if script == "plot_activations" else []))
    with pytest.raises(SystemExit, match="--u8_input"):
        mod.run(args)


# ---- GPU suite ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_op(hip):
    FC.check_shapes(hip, "cuda")
    FC.check_indexed(hip, "cuda")
    FC.check_accumulate(hip, "cuda")
    FC.check_blocks(hip, "cuda")
    FC.check_saturated(hip, "cuda")
    FC.check_errors(hip, "cuda")


@pytest.mark.gpu
def test_gpu_op_192_saturated_frames_one_workgroup(hip):
    """192 saturated frames of 256x341 (50 MB) through ONE workgroup: 65 472 bytes of 255 per channel for each of its 256 lanes"""
    FC.check_saturated(hip, "cuda", n=192, h=256, w=341, blocks=1)


@pytest.mark.gpu
def test_gpu_op_lane_accumulators_are_widened_in_time(hip):
    FC.check_saturated(hip, "cuda", *WIDEN_CASE, blocks=1)


@pytest.mark.gpu
def test_gpu_pixel_sums(hip):
    FC.check_sources(hip, "cuda")
    FC.check_resize(hip, "cuda")
    FC.check_against_reference(hip, "cuda")
