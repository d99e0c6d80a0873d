#!/usr/bin/env python
"""Cost of the inference input gradient (mn_input_grad) on an MI355X: the whole call beside the eval forward pass of the same
plan, and the stem data gradient (mn_op_stem_dgrad) per launch, at 256 x 341, fp32 and fp16, B = 1 and B = 192.

Every figure is the median of `--rounds` event-timed bursts of `--iters` calls after a warm-up, the two arms of a pair interleaved
in one process.  Prints one JSON line per (dtype, batch) and writes them to --out."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 192])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=341)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import statistics
    import torch
    import geomapnet_amd as G
    from geomapnet_amd import _binding
    from geomapnet_amd._binding import ptr
    lib = _binding.hip()
    H, W = args.height, args.width
    H0, W0 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = []
    for dt in args.dtypes:
        G.set_compute_dtype(dt)
        torch.manual_seed(7)
        net = G.PoseNet(G.resnet34(), droprate=0.0, pretrained=False).cuda().eval()
        td, code = (torch.float16, 1) if dt == "fp16" else (torch.float32, 0)
        w = torch.randn(64, 7, 7, 3, device="cuda") * 0.1
        for B in args.batches:
            x = torch.randn(B, 3, H, W, device="cuda")
            gy = torch.randn(B, H0, W0, 64, device="cuda").to(td)
            gx = torch.empty(B, 3, H, W, device="cuda")
            arms = {"forward_ms": lambda: net(x), "input_grad_ms": lambda: net.input_gradient(x), "saliency_ms": lambda: net.saliency(x),
                    "stem_dgrad_ms": lambda: lib.check(lib.op_stem_dgrad(code, ptr(gy), ptr(w), ptr(gx), B, H, W, C.c_float(1.0), None))}
            for fn in arms.values():  # warm-up: plans, weight repack, clocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    t[k].append(timed(fn, args.iters, torch))
            row = {"dtype": dt, "B": B, "H": H, "W": W}
            for k, v in t.items():
                row[k] = round(statistics.median(v), 4)
                row[k.replace("_ms", "_min_ms")] = round(min(v), 4)
            row["stem_dgrad_tmacs"] = round(B * H0 * W0 * 64 * 147 / (row["stem_dgrad_ms"] * 1e-3) / 1e12, 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
