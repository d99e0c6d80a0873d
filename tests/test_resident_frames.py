"""Device-resident frame store (csrc/gather.h, the indexed resize_u8_kernel, mn_set_input_index, geomapnet_amd/resident.py): batches
gathered by index in HBM instead of stacked on the host.  Gathering is a copy, so every comparison is bit for bit against the tensor
`store[index]` (tests/resident_checks.py).  CPU tests run the kernels in the SIMT emulator; the GPU tests (-m gpu) run them on
libmapnet_hip.so, with a store above 4 GiB too.  The bounds guard is exercised in the emulator only."""
import configparser
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu_lib
import resident_checks as K
from geomapnet_amd import resident
from geomapnet_amd._binding import MapNetHipError
from geomapnet_amd.data import MF, MFOnline, SyntheticFrames, calc_vos_safe
from geomapnet_amd.resident import ResidentFrames, ResidentLoader
from geomapnet_amd.trainer import safe_collate

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


_IDS = ["4653", "6360", "3840", "fp32-18612"]

# ---- operators: CPU suite (SIMT emulator) ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", K.GATHER_CASES, ids=_IDS)
def test_op_gather_frames(emu, case):
    K.check_gather_case(emu, "cpu", case)


@pytest.mark.parametrize("sh,sw,H,W", K.RESIZE_CASES)
def test_op_resize_indexed(emu, sh, sw, H, W):
    K.check_resize_indexed(emu, "cpu", sh, sw, H, W)


def test_bounds_guard(emu):
    K.check_bounds_guard(emu, "cpu")


# ---- plans: CPU suite ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fp32", "u8", "u8_resize", "u8_jitter"])
def test_plan_forward(emu, form):
    K.check_plan_forward(emu, "cpu", "fp32", form)


def test_plan_train_step(emu):
    K.check_plan_train_step(emu, "cpu", "fp32")


def test_plan_input_gradient_and_saliency(emu):
    K.check_plan_input_grad(emu, "cpu", "fp32")


def test_off_is_off(emu):
    K.check_off_is_off(emu, "cpu")


# ---- host logic: the loader (device cpu, no kernels) ------------------------------------------------------------------------------
def _cases():
    u8 = dict(H=32, W=40, uint8=True)
    yield "fixed_skip", lambda: [SyntheticFrames(9, **u8)], lambda f: MF(f[0], steps=3, skip=2)
    yield "variable_skip", lambda: [SyntheticFrames(9, **u8)], lambda f: MF(f[0], steps=3, skip=2, variable_skip=True)
    yield ("vos_real", lambda: [SyntheticFrames(9, **u8), SyntheticFrames(9, seed=8, **u8)],
           lambda f: MF(f[0], steps=3, skip=2, include_vos=True, real=True, vo_func=calc_vos_safe, gt_dataset=f[1]))
    yield ("online", lambda: [SyntheticFrames(5, **u8), SyntheticFrames(7, seed=9, **u8)],
           lambda f: MFOnline(f[0], f[1], val_gt_dataset=f[1], steps=3, skip=2))


LOADER_CASES = list(_cases())


@pytest.mark.parametrize("name,make_frames,make_windows", LOADER_CASES, ids=[c[0] for c in LOADER_CASES])
def test_loader_equivalence(name, make_frames, make_windows):
    frames = make_frames()
    host_set = make_windows(frames)
    views = ResidentFrames.build(frames, "cpu")
    assert all(v.store is views[0].store for v in views)
    assert [v.base for v in views] == list(np.cumsum([0] + [len(f) for f in frames[:-1]]))
    for f, v in zip(frames, views):  # a view is itself a frame dataset
        assert len(v) == len(f) and torch.equal(v.poses, f.poses) and v.gt_idx is f.gt_idx
        img, pose = v[len(f) - 1]
        assert torch.equal(img, f[len(f) - 1][0]) and torch.equal(pose, f[len(f) - 1][1])
    res_set = make_windows(views)
    store = views[0].store
    batches = {}
    for seed in (0, 5):
        for kind in ("host", "resident"):
            torch.manual_seed(seed)
            np.random.seed(seed)
            if kind == "host":
                loader = torch.utils.data.DataLoader(host_set, batch_size=4, shuffle=True, num_workers=0, collate_fn=safe_collate)
                batches[kind] = [(d, t) for d, t in loader]
            else:
                loader = ResidentLoader(res_set, batch_size=4, shuffle=True, device="cpu")
                batches[kind] = [(d.gather(), t, d) for d, t in loader]
            batches[kind + "_len"] = len(loader)
        assert batches["host_len"] == batches["resident_len"] == len(batches["host"]) == len(batches["resident"])
        assert len(host_set) % 4 != 0 and batches["host"][-1][0].shape[0] == len(host_set) % 4  # a last partial batch
        for (d, t), (rd, rt, frames_) in zip(batches["host"], batches["resident"]):
            assert frames_.index.dtype == torch.int32 and tuple(frames_.shape) == tuple(d.shape)
            assert torch.equal(rd, d), name
            assert rt.dtype == t.dtype and torch.equal(rt, t), name


def test_posenet_frames_through_the_loader():
    frames = SyntheticFrames(6, H=32, W=40, uint8=True)
    (view,) = ResidentFrames.build([frames], "cpu")
    torch.manual_seed(1)
    host = list(torch.utils.data.DataLoader(frames, batch_size=4, shuffle=True, num_workers=0, collate_fn=safe_collate))
    torch.manual_seed(1)
    res = list(ResidentLoader(view, batch_size=4, shuffle=True, device="cpu"))
    assert len(host) == len(res) == 2
    for (d, t), (r, rt) in zip(host, res):
        assert tuple(r.shape) == tuple(d.shape) and torch.equal(r.gather(), d) and torch.equal(rt, t)


def test_build_refuses_a_store_larger_than_free_memory(monkeypatch):
    frames = SyntheticFrames(9, H=32, W=40, uint8=True)
    need = 9 * 32 * 40 * 3
    monkeypatch.setattr(resident, "free_memory", lambda device: need - 1)

    def no_alloc(*a, **k):
        raise AssertionError("the store was allocated")

    monkeypatch.setattr(torch, "empty", no_alloc)
    with pytest.raises(MapNetHipError) as e:
        ResidentFrames.build([frames], "cpu")
    assert str(need) in str(e.value) and str(need - 1) in str(e.value)


def test_build_refuses_mixed_frames():
    with pytest.raises(ValueError, match="the store holds"):
        ResidentFrames.build([SyntheticFrames(2, H=32, W=40, uint8=True), SyntheticFrames(2, H=32, W=48, uint8=True)], "cpu")
    with pytest.raises(ValueError, match="the store holds"):
        ResidentFrames.build([SyntheticFrames(2, H=32, W=40, uint8=True), SyntheticFrames(2, H=32, W=40)], "cpu")


# ---- Trainer and scripts/train.py on the emulator ---------------------------------------------------------------------------------
def _train(emu, tmp_path, tag, extra):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train as train_script
    s = configparser.ConfigParser()
    s.read(os.path.join(ROOT, "scripts", "configs", "synthetic_mapnet.ini"))
    s["training"].update(n_epochs="1", batch_size="2", snapshot="1", val_freq="1", do_val="yes")
    s["hyperparameters"]["skip"] = "1"
    os.makedirs(str(tmp_path / tag), exist_ok=True)  # (a directory per run: runs may go side by side)
    cfg = str(tmp_path / tag / "synthetic_mapnet.ini")
    with open(cfg, "w") as f:
        s.write(f)
    argv = ["--model", "mapnet", "--config_file", cfg, "--dtype", "fp32", "--synthetic_length", "2", "--synthetic_val_length", "2",
            "--height", "32", "--width", "40", "--logdir", str(tmp_path / ("logs_" + tag)), "--num_workers", "0", "--u8_input"]
    lines = []
    tr = train_script.run(train_script.build_parser().parse_args(argv + list(extra)), _binding=emu, log=lines.append)
    losses = [re.search(r"(Loss|val_loss) (\S+)", l).group(2) for l in lines if l.startswith(("Train ", "Val "))]
    return tr, lines, losses


def _same_checkpoints(dir_a, dir_b):
    for e in (0, 1):
        ca = torch.load(os.path.join(dir_a, "epoch_%03d.pth.tar" % e), weights_only=False)
        cb = torch.load(os.path.join(dir_b, "epoch_%03d.pth.tar" % e), weights_only=False)
        assert ca["epoch"] == cb["epoch"]
        for k, v in ca["model_state_dict"].items():
            assert torch.equal(v, cb["model_state_dict"][k]), k
        for k, v in ca["criterion_state_dict"].items():
            assert torch.equal(v, cb["criterion_state_dict"][k]), k
        sa, sb = ca["optim_state_dict"]["state"], cb["optim_state_dict"]["state"]
        assert sa.keys() == sb.keys()
        for k in sa:
            for name, v in sa[k].items():
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb[k][name])), (k, name)


def _arm_main(tmp, tag, extra):
    """one training run in a process of its own (see test_train_script_flag); prints one JSON line"""
    import json
    import pathlib
    tr, lines, losses = _train(emu_lib.load(), pathlib.Path(tmp), tag, extra)
    store = tr.frame_store
    print("ARM " + json.dumps({"losses": losses, "logdir": tr.logdir, "train_loader": type(tr.train_loader).__name__,
                               "val_loader": type(tr.val_loader).__name__,
                               "store": None if store is None else [list(store.shape), str(store.dtype)],
                               "store_line": [l for l in lines if l.startswith("Resident frame store")]}))


def _spawn_arm(tmp_path, tag, extra):
    env = dict(os.environ, MN_DETERMINISTIC="1",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    code = "import test_resident_frames as t; t._arm_main(%r, %r, %r)" % (str(tmp_path), tag, list(extra))
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_train_script_flag(emu, tmp_path):
    """train.run(--u8_input --resident_frames) logs the losses and writes the checkpoints of the run without the flag.  Two runs of
    the host loader in one process print the same losses to six decimals but do NOT write the same checkpoints (float atomics in
    an order that changes from run to run; tried on the emulator: conv1.weight differs after the step), so both arms run under
    MN_DETERMINISTIC=1, each in a child process of its own -- the knob table is process-wide -- and side by side."""
    import json
    procs = [_spawn_arm(tmp_path, "host", []), _spawn_arm(tmp_path, "resident", ["--resident_frames"])]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    host, res = (json.loads([l for l in o.splitlines() if l.startswith("ARM ")][-1][4:]) for o in outs)
    assert host["train_loader"] == host["val_loader"] == "DataLoader" and host["store"] is None  # without the flag: as before
    assert res["train_loader"] == res["val_loader"] == "ResidentLoader"
    assert res["store"] == [[4, 32, 40, 3], "torch.uint8"]
    assert len(res["store_line"]) == 1 and res["store_line"][0].startswith("Resident frame store: 4 frames")
    assert len(host["losses"]) == 3 and res["losses"] == host["losses"]
    _same_checkpoints(host["logdir"], res["logdir"])


# ---- GPU suite ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", K.GATHER_CASES, ids=_IDS)
def test_gpu_op_gather_frames(hip, case):
    K.check_gather_case(hip, "cuda", case)


@pytest.mark.gpu
@pytest.mark.parametrize("sh,sw,H,W", K.RESIZE_CASES)
def test_gpu_op_resize_indexed(hip, sh, sw, H, W):
    K.check_resize_indexed(hip, "cuda", sh, sw, H, W)


@pytest.mark.gpu
def test_gpu_store_above_4gib(hip):
    K.check_store_above_4gib(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "fp16x2m"])
@pytest.mark.parametrize("form", ["fp32", "u8", "u8_resize", "u8_jitter"])
def test_gpu_plan_forward(hip, dtype_name, form):
    K.check_plan_forward(hip, "cuda", dtype_name, form)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "fp16x2m"])
def test_gpu_plan_train_step(hip, dtype_name):
    K.check_plan_train_step(hip, "cuda", dtype_name)


@pytest.mark.gpu
def test_gpu_plan_input_gradient_and_saliency(hip):
    K.check_plan_input_grad(hip, "cuda", "fp32")


@pytest.mark.gpu
def test_gpu_off_is_off(hip):
    K.check_off_is_off(hip, "cuda", other_device="cpu")
