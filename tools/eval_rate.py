"""Inference rate of the fused inference pass (model.set_eval_fused, include/mapnet_hip.h mn_set_eval_fused) against the unfused pass
on the MI355X, fp16x2m, in ONE process with the two arms alternating on ONE model (the switch is flipped between regions):
  * 64 windows x T=3 = 192 images of 256x341, the BASELINE configs[2] batch;
  * one window of T=3 at 256x341, what scripts/eval.py runs per loader item, where the launch count dominates.
A region = `passes` eval-mode forward passes between two device synchronisations, wall clock; each arm is warmed up, then `rounds`
regions per arm alternate (the order flips every round).  Reported per arm: the median region (ms per pass, images/s) and the
region-to-region spread (max - min); a difference between the arms is real only where it exceeds that spread.  Both arms must give
the same poses bit for bit, or the tool fails.
usage: python tools/eval_rate.py [--rounds R] [--out profiles/r07/fused_eval.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geomapnet_amd as G  # noqa: E402

SHAPES = (("192 images (64 windows x T=3) of 256x341, BASELINE configs[2]", 64, 64), ("one window of T=3 at 256x341 (scripts/eval.py)", 1, 400))


def measure(name, windows, passes, args):
    torch.manual_seed(3)
    net = G.MapNet(G.PoseNet(G.resnet34(), droprate=0.0, pretrained=False))
    net.cuda()
    net.eval()
    x = torch.randn(windows, 3, 3, args.height, args.width, generator=torch.Generator().manual_seed(11)).cuda()

    def region(fused, n):
        net.set_eval_fused(fused)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(n):
                poses = net(x)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, poses

    arms = {"unfused": False, "fused": True}
    last = {}
    for arm, fused in arms.items():  # warm-up of each arm (plan creation, weight repack, clocks)
        _, last[arm] = region(fused, max(3, passes // 2))
    assert torch.equal(last["unfused"], last["fused"]), "the fused pass must give the unfused pass's poses bit for bit"
    ms = {arm: [] for arm in arms}
    order = list(arms)
    for r in range(args.rounds):
        for arm in (order if r % 2 == 0 else order[::-1]):
            t, _ = region(arms[arm], passes)
            ms[arm].append(t)
    images = windows * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    d = med["fused"] - med["unfused"]
    return {"what": "eval-mode forward pass, fp16x2m, %s; %d regions of %d passes per arm, alternating" % (name, args.rounds, passes),
            "ms_per_pass": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "median_ms_per_pass": {k: round(v, 4) for k, v in med.items()},
            "images_per_s": {k: round(1e3 * images / v, 1) for k, v in med.items()},
            "spread_ms": {k: round(v, 4) for k, v in spread.items()},
            "fused_minus_unfused_ms": round(d, 4), "fused_minus_unfused_pct": round(100 * d / med["unfused"], 2),
            "difference_exceeds_spread": abs(d) > max(spread.values()), "poses_bit_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="timed regions per arm (at least 5)")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=341)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least five regions per arm"
    assert torch.cuda.is_available(), "eval_rate.py measures the MI355X; there is no CPU fallback"
    G.set_compute_dtype("fp16x2m")
    lines = [json.dumps(measure(name, windows, passes, args)) for name, windows, passes in SHAPES]
    for ln in lines:
        print(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
