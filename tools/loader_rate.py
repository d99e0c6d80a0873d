"""The loader-inclusive rate of the BASELINE configs[2] training step (64 windows x T=3 = 192 uint8 frames, default dtype): what
bench.py's `input_feed` does not measure -- it starts from batches already assembled in pinned memory.  Frames are held in host memory
as one uint8 array (generated once, not per __getitem__); windows are MF(steps=3, skip=10) over them, shuffled.
  arms     host0, host8   the parent's path: DataLoader(num_workers 0 / 8, pin_memory, safe_collate) + DeviceFeed
           resident       ResidentFrames.build + ResidentLoader (geomapnet_amd/resident.py)
  sizes    256x341 (pre-resized frames) and 480x640 with the device Resize(256)
Per arm: images/s over the timed steps (host clock around steps that end in a device synchronise) and the loop's data-wait time per
step (host time blocked in next(loader), as Trainer's "Data time").
  --part rate      all arms at one frame size, one JSON line per arm
  --part profile   a few gathers, plain and indexed resizes, untimed: for
                   `rocprofv3 --kernel-trace --stats -- python tools/loader_rate.py --part profile`
usage: python tools/loader_rate.py --part rate --size 256x341|480x640 [--steps 200] [--arms host0,host8,resident]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geomapnet_amd as G  # noqa: E402
from geomapnet_amd import _binding  # noqa: E402
from geomapnet_amd._binding import ptr  # noqa: E402
from geomapnet_amd.data import MF, resize_dims  # noqa: E402
from geomapnet_amd.trainer import safe_collate  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class HostFrames(torch.utils.data.Dataset):
    """L decoded frames in host memory, uint8 [L, h, w, 3], generated once; poses on a random walk"""

    def __init__(self, length, h, w, seed=1):
        rng = np.random.default_rng(seed)
        self.images = torch.from_numpy(rng.integers(0, 256, (length, h, w, 3), dtype=np.uint8))
        g = torch.Generator().manual_seed(seed)
        self.poses = torch.cumsum(0.05 * torch.randn(length, 6, generator=g), dim=0)
        self.gt_idx = np.arange(length)

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        return self.images[int(i)], self.poses[int(i)]


def build(resize):
    torch.manual_seed(3)
    net = G.MapNet(G.PoseNet(G.resnet34(), droprate=0.0, pretrained=False))
    crit = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True)
    net.cuda()
    crit.cuda()
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [crit.sax, crit.saq]}, {"params": [crit.srx, crit.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    net.train()
    net.set_input_u8(MEAN, STD)
    if resize is not None:
        net.set_input_resize(resize)
    return net, crit, opt


def batches(loader):
    """an endless stream of the loader's batches (epoch after epoch)"""
    while True:
        for b in loader:
            yield b


def run_arm(name, frames, args, model):
    net, crit, opt = model
    if name == "resident":
        t0 = time.perf_counter()
        (view,) = G.ResidentFrames.build([frames], "cuda")
        torch.cuda.synchronize()
        upload = time.perf_counter() - t0
        loader = G.ResidentLoader(MF(view, steps=3, skip=10), batch_size=args.windows, shuffle=True, drop_last=True, device="cuda")
    else:
        upload = 0.0
        workers = int(name[4:])
        host = torch.utils.data.DataLoader(MF(frames, steps=3, skip=10), batch_size=args.windows, shuffle=True, drop_last=True,
                                           num_workers=workers, pin_memory=True, collate_fn=safe_collate,
                                           persistent_workers=workers > 0)
        loader = G.DeviceFeed(host, "cuda")
    it = batches(loader)
    for _ in range(args.warmup):
        x, t = next(it)
        loss, _ = G.step_feedfwd(x, net, True, t, crit, opt, True)
    torch.cuda.synchronize()
    wait = 0.0
    t_start = time.perf_counter()
    for _ in range(args.steps):
        t0 = time.perf_counter()
        x, t = next(it)
        wait += time.perf_counter() - t0
        loss, _ = G.step_feedfwd(x, net, True, t, crit, opt, True)
    torch.cuda.synchronize()
    total = time.perf_counter() - t_start
    assert np.isfinite(loss)
    del it, loader
    images = args.steps * args.windows * 3
    return {"arm": name, "frame": "%dx%d" % tuple(frames.images.shape[1:3]), "steps": args.steps, "images_per_s": round(images / total, 1),
            "ms_per_step": round(1e3 * total / args.steps, 3), "data_wait_ms_per_step": round(1e3 * wait / args.steps, 3),
            "store_upload_s": round(upload, 2), "frames_in_sequence": len(frames), "dtype": G.get_compute_dtype()}


def part_rate(args):
    h, w = (int(v) for v in args.size.split("x"))
    resize = args.resize if (h, w) != resize_dims(h, w, args.resize) else None
    frames = HostFrames(args.frames, h, w)
    model = build(resize)  # one model for every arm: the same kernels, the same plans
    for name in args.arms.split(","):
        print(json.dumps(run_arm(name, frames, args, model)), flush=True)


def part_profile(args):
    lib = _binding.hip()
    B, F = args.windows * 3, args.frames
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(1)
    idx = torch.randint(0, F, (B,), generator=gen, dtype=torch.int32).cuda()
    flag = torch.zeros(1, device="cuda")
    small = torch.randint(0, 256, (F, 256, 341, 3), generator=gen, dtype=torch.uint8).cuda()
    out = torch.empty(B, 256, 341, 3, dtype=torch.uint8, device="cuda")
    big = torch.randint(0, 256, (F, 480, 640, 3), generator=gen, dtype=torch.uint8).cuda()
    batch = big[idx.long()].contiguous()
    work = torch.empty(int(lib.op_resize_work_bytes(480, 640, 256, 341)), dtype=torch.uint8, device="cuda")
    for _ in range(args.reps):
        lib.check(lib.op_gather_frames(ptr(small), ptr(idx), ptr(out), 256 * 341 * 3, B, F, ptr(flag), s))
        lib.check(lib.op_resize_u8(ptr(batch), ptr(out), ptr(work), B, 480, 640, 256, 341, s))
        lib.check(lib.op_resize_u8_indexed(ptr(big), ptr(idx), F, ptr(out), ptr(work), B, 480, 640, 256, 341, ptr(flag), s))
    torch.cuda.synchronize()
    assert flag.item() == 0.0
    print("profile run: %d x (gather of %d frames 256x341 from %d; plain resize; indexed resize of 480x640 -> 256x341)" % (args.reps, B, F))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("rate", "profile"), required=True)
    ap.add_argument("--size", default="256x341", help="frame size held by the sequence: 256x341, or 480x640 (device Resize)")
    ap.add_argument("--resize", type=int, default=256)
    ap.add_argument("--arms", default="host0,host8,resident")
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000, help="frames in the sequence (a small 7Scenes scene)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20, help="part profile: launches of each kernel")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loader_rate.py measures the MI355X; there is no CPU fallback"
    if args.part == "rate":
        part_rate(args)
    else:
        part_profile(args)


if __name__ == "__main__":
    main()
