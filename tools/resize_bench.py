"""What the device Resize (csrc/resize.h) costs at BASELINE configs[2]: 64 windows x T=3 = 192 uint8 frames of 480x640 (7Scenes)
resampled to 256x341 on the MI355X.
  --part a        the conversion alone (mn_op_resize_u8): HIP events around each call, median; against its byte floor (source +
                  output once each).  The interval holds the call's table upload (a few KB) as well as the kernel.
  --part b        the fp16x2m training step on 480x640 frames resized on the device against the same step on pre-resized 256x341
                  frames, both resident on the device: two models, alternating timed regions on the same box
  --part c        the same pair through DeviceFeed from pinned host memory (the copy grows from 50 MB to 177 MB per step)
  --part profile  a few conversions, untimed: for `rocprofv3 --kernel-trace --stats -- python tools/resize_bench.py --part profile`
usage: python tools/resize_bench.py --part a|b|c|profile [--steps K] [--rounds R]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geomapnet_amd as G  # noqa: E402
from geomapnet_amd import _binding  # noqa: E402
from geomapnet_amd._binding import ptr  # noqa: E402
from geomapnet_amd.data import resize_dims  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def part_a(args, profile=False):
    lib = _binding.hip()
    B, sh, sw = args.windows * 3, args.src_height, args.src_width
    H, W = resize_dims(sh, sw, args.size)
    gen = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (B, sh, sw, 3), generator=gen, dtype=torch.uint8).cuda()
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
    work = torch.empty(int(lib.op_resize_work_bytes(sh, sw, H, W)), dtype=torch.uint8, device="cuda")
    th, tw = C.c_int(), C.c_int()
    lib.check(lib.op_resize_tile(sh, sw, H, W, C.byref(th), C.byref(tw)))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        lib.check(lib.op_resize_u8(ptr(x), ptr(out), ptr(work), B, sh, sw, H, W, s))

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    if profile:
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        print("profile run: 20 conversions of %d frames %dx%d -> %dx%d" % (B, sh, sw, H, W))
        return
    us = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    # back to back: the table upload and the launch of call k+1 hide under the kernel of call k
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        call()
    e1.record()
    e1.synchronize()
    floor = x.numel() + out.numel()
    med = statistics.median(us)
    b2b = 1e3 * e0.elapsed_time(e1) / args.reps
    print(json.dumps({"what": "mn_op_resize_u8, %d frames %dx%d -> %dx%d, tile %d rows x %d columns" % (B, sh, sw, H, W, th.value, tw.value),
                      "us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "reps": args.reps,
                      "us_back_to_back": round(b2b, 1), "floor_bytes": floor,
                      "GBps_of_floor_median": round(floor / med / 1e3, 1), "GBps_of_floor_back_to_back": round(floor / b2b / 1e3, 1)}))


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


def part_bc(args, feed):
    G.set_compute_dtype(args.dtype)
    n, T, sh, sw = args.windows, 3, args.src_height, args.src_width
    H, W = resize_dims(sh, sw, args.size)
    gen = torch.Generator().manual_seed(11)
    legs = {}
    for name, (h, w, size) in (("pre_resized", (H, W, None)), ("device_resize", (sh, sw, args.size))):
        xs = [torch.randint(0, 256, (n, T, h, w, 3), generator=gen, dtype=torch.uint8) for _ in range(2)]
        ts = [torch.randn(n, T, 6, generator=gen) * 0.3 for _ in range(2)]
        if feed:
            xs, ts = [x.pin_memory() for x in xs], [t.pin_memory() for t in ts]
        else:
            xs, ts = [x.cuda() for x in xs], [t.cuda() for t in ts]
        legs[name] = (build(size), xs, ts)

    def region(name, steps):
        (net, crit, opt), xs, ts = legs[name]
        batches = [(xs[k % 2], ts[k % 2]) for k in range(steps)]
        src = G.DeviceFeed(batches, "cuda") if feed else batches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for x, t in src:
            loss, _ = G.step_feedfwd(x, net, True, t, crit, opt, True)
        torch.cuda.synchronize()
        assert torch.isfinite(torch.tensor(float(loss)))
        return 1e3 * (time.perf_counter() - t0) / steps

    for name in legs:
        region(name, 6)
    res = {name: [] for name in legs}
    names = list(legs)
    for r in range(args.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            res[name].append(region(name, args.steps))
    m = {k: statistics.median(v) for k, v in res.items()}
    d = m["device_resize"] - m["pre_resized"]
    print(json.dumps({"what": "BASELINE configs[2] training step, %d x %d uint8 frames, %s, %s: %dx%d frames resized on the device to %dx%d "
                              "against pre-resized frames, alternating regions of %d steps"
                              % (n, T, args.dtype, "through DeviceFeed from pinned memory" if feed else "frames resident on the device",
                                 sh, sw, H, W, args.steps),
                      "ms_per_step": {k: [round(x, 3) for x in v] for k, v in res.items()},
                      "median_ms": {k: round(v, 3) for k, v in m.items()}, "delta_ms": round(d, 3),
                      "delta_pct": round(100 * d / m["pre_resized"], 2),
                      "spread_ms": {k: round(max(v) - min(v), 3) for k, v in res.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b", "c", "profile"), required=True)
    ap.add_argument("--dtype", default="fp16x2m")
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--src_height", type=int, default=480)
    ap.add_argument("--src_width", type=int, default=640)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30, help="part a: timed conversions")
    ap.add_argument("--steps", type=int, default=16, help="parts b, c: steps per timed region")
    ap.add_argument("--rounds", type=int, default=6, help="parts b, c: region pairs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resize_bench.py measures the MI355X; there is no CPU fallback"
    if args.part in ("a", "profile"):
        part_a(args, profile=args.part == "profile")
    else:
        part_bc(args, feed=args.part == "c")


if __name__ == "__main__":
    main()
