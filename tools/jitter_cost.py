"""What the device ColorJitter (csrc/jitter.h) costs the training step at BASELINE configs[2]: MapNet, ResNet-34, 64 windows x T=3
= 192 uint8 frames of 256x341 resident on the device, fp16x2m, MapNet criterion, Adam.  One model, jitter off and on (the
reference's ColorJitter(0.7, 0.7, 0.7, hue=0.5)) in alternating timed regions, so both legs see the same box and the same clocks.
usage: python tools/jitter_cost.py [--steps K] [--rounds R] [--dtype fp16x2m]
       python tools/jitter_cost.py --profile_steps 6   (a few jittered steps, no timing: for rocprofv3 --kernel-trace --stats)"""
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

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CJ = 0.7  # scripts/configs/synthetic_mapnet.ini and the reference's mapnet.ini


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16x2m")
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=341)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed region")
    ap.add_argument("--rounds", type=int, default=8, help="off / on region pairs")
    ap.add_argument("--profile_steps", type=int, default=0, help="run this many jittered steps untimed and exit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jitter_cost.py measures the MI355X; there is no CPU fallback"
    G.set_compute_dtype(args.dtype)
    torch.manual_seed(3)
    net = G.MapNet(G.PoseNet(G.resnet34(), droprate=0.0, pretrained=False))
    crit = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True)
    net.cuda()
    crit.cuda()
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [crit.sax, crit.saq]}, {"params": [crit.srx, crit.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    net.train()
    net.set_input_u8(MEAN, STD)
    n, T, H, W = args.windows, 3, args.height, args.width
    gen = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (n, T, H, W, 3), generator=gen, dtype=torch.uint8).cuda()
    t = (torch.randn(n, T, 6, generator=gen) * 0.3).cuda()

    def jitter(on):
        if on:
            net.set_color_jitter(CJ, CJ, CJ, 0.5, seed=5)
        else:
            net.set_color_jitter()

    def region(on, steps):
        jitter(on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss, _ = G.step_feedfwd(x, net, True, t, crit, opt, True)
        torch.cuda.synchronize()
        assert torch.isfinite(torch.tensor(float(loss)))
        return 1e3 * (time.perf_counter() - t0) / steps

    if args.profile_steps:
        region(False, 3)
        region(True, args.profile_steps)
        print("profile run: %d jittered steps" % args.profile_steps)
        return
    region(False, 8)  # warm-up of both legs
    region(True, 8)
    off, on = [], []
    for r in range(args.rounds):
        order = (False, True) if r % 2 == 0 else (True, False)
        for leg in order:
            (on if leg else off).append(region(leg, args.steps))
    m_off, m_on = statistics.median(off), statistics.median(on)
    print(json.dumps({"what": "BASELINE configs[2] training step, %d x %d uint8 frames %dx%d resident, %s; ColorJitter(%.1f, %.1f, %.1f, "
                              "hue=0.5) on the device off / on in alternating regions of %d steps" % (n, T, H, W, args.dtype, CJ, CJ,
                                                                                                      CJ, args.steps),
                      "ms_per_step_off": [round(v, 3) for v in off], "ms_per_step_on": [round(v, 3) for v in on],
                      "median_off": round(m_off, 3), "median_on": round(m_on, 3), "delta_ms": round(m_on - m_off, 3),
                      "delta_pct": round(100 * (m_on - m_off) / m_off, 2),
                      "spread_off_ms": round(max(off) - min(off), 3), "spread_on_ms": round(max(on) - min(on), 3)}))


if __name__ == "__main__":
    main()
