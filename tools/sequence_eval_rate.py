"""Wall time of sequence evaluation (geomapnet_amd.evaluate.evaluate_sequence: every frame forwarded once, windows and VOs assembled on
the device) against the window loop (evaluate over a batch-size-1 DataLoader, what scripts/eval.py runs) on the MI355X, in ONE process
on ONE model: fp16x2m, uint8 input, the fused inference pass on.  The data is a synthetic uint8 sequence of `--frames` frames of
256x341 held in host memory.  Two cells:
  * steps=3, skip=10 (mapnet.ini), no pose graph;
  * steps=7, skip=10 with the pose graph on all pairs (pgo_inference_*.ini with fc_vos), scattered by get_indices.
Three arms per cell: `loop`, `sequence` fed from the host dataset, `sequence_resident` fed by index from a ResidentFrames store (built
outside the timed regions).  A region = one whole evaluation, wall clock between two device synchronisations; each arm is warmed up,
then `rounds` regions per arm alternate (the order flips every round).  Reported per arm: the median region, the region-to-region spread
(max - min) and the median split of the wall time into pose-graph optimisation (optimize_windows / optimize_windows_dev, with their
copies and the status read-back), host post-processing (to_pose7, the VO function, scatter and error statistics) and forward = the
rest (loader, host-to-device copies, launches, device-to-host copies).  The arms must agree within the bounds of
tests/seq_eval_checks.py, or the tool fails.
usage: python tools/sequence_eval_rate.py [--rounds R] [--frames L] [--out profiles/r07/sequence_eval.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geomapnet_amd as G  # noqa: E402
from geomapnet_amd import evaluate as E  # noqa: E402
from geomapnet_amd import pgo as P  # noqa: E402
from geomapnet_amd.data import MF, SyntheticFrames, calc_vos_safe_fc  # noqa: E402
from geomapnet_amd.resident import make_resident  # noqa: E402

CELLS = (("steps=3, skip=10, no pose graph", 3, False), ("steps=7, skip=10, pose graph on all pairs (fc_vos)", 7, True))
SIG = dict(sax=1.0, saq=1.0, srx=20.0, srq=20.0)


class MemFrames(torch.utils.data.Dataset):
    """decoded frames in host memory: uint8 [L,H,W,3], poses of SyntheticFrames"""

    def __init__(self, length, H, W, seed=7):
        self.images = torch.randint(0, 256, (length, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
        self.poses = SyntheticFrames(length, H=8, W=8, seed=seed).poses
        self.gt_idx = np.arange(length)

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[int(i)], self.poses[int(i)]


class Split:
    """seconds spent inside the wrapped functions, per category; nested calls of one category count once"""

    def __init__(self):
        self.t, self.depth = {"host": 0.0, "pgo": 0.0}, {"host": 0, "pgo": 0}

    def wrap(self, fn, cat):
        def timed(*a, **k):
            self.depth[cat] += 1
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.depth[cat] -= 1
                if self.depth[cat] == 0:
                    self.t[cat] += time.perf_counter() - t0
        return timed


def region(arm, net, sets, pose_graph, args):
    """one evaluation -> (wall s, split, (summary, pred, targ))"""
    split = Split()
    saved = (E.to_pose7, E._scatter_and_summarize, P.optimize_windows, P.optimize_windows_dev)
    E.to_pose7, E._scatter_and_summarize = split.wrap(saved[0], "host"), split.wrap(saved[1], "host")
    P.optimize_windows, P.optimize_windows_dev = split.wrap(saved[2], "pgo"), split.wrap(saved[3], "pgo")
    mf = sets["resident" if arm == "sequence_resident" else "host"]
    vo_func = mf.vo_func
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if arm == "loop":
            mf.vo_func = split.wrap(vo_func, "host")  # (MF.__getitem__ calls it; the sequence arms never do)
            loader = torch.utils.data.DataLoader(mf, batch_size=1, shuffle=False, num_workers=0, pin_memory=True)
            out = E.evaluate(net, loader, cuda=True, pose_graph=pose_graph, fc_vos=pose_graph,
                             indices_of=mf.get_indices if pose_graph else None, length=len(mf) if pose_graph else None, **SIG)
        else:
            out = E.evaluate_sequence(net, mf, cuda=True, pose_graph=pose_graph, fc_vos=pose_graph, batch_frames=args.batch_frames,
                                      scatter=pose_graph, **SIG)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        mf.vo_func = vo_func
        E.to_pose7, E._scatter_and_summarize, P.optimize_windows, P.optimize_windows_dev = saved
    return wall, {"forward": wall - split.t["host"] - split.t["pgo"], "host": split.t["host"], "pgo": split.t["pgo"]}, out


def agree(ref, got, pose_graph, exact=False):
    """the bounds of tests/seq_eval_checks.py (pose_s = 1 here)"""
    (s0, p0, t0), (s1, p1, t1) = ref, got
    assert p0.shape == p1.shape and np.array_equal(t0, t1), "targets differ"
    if exact:
        assert np.array_equal(p0, p1), "host-fed and resident sequence evaluation must agree bit for bit"
    elif pose_graph:
        np.testing.assert_allclose([s1["median_t"], s1["mean_t"]], [s0["median_t"], s0["mean_t"]], rtol=2e-3, atol=2e-3)
    else:
        bound = 2 * 1e-3 * max(1.0, float(np.abs(p0[:, :3]).max()))
        assert np.abs(p0[:, :3] - p1[:, :3]).max() <= bound, (np.abs(p0[:, :3] - p1[:, :3]).max(), bound)


def measure(name, steps, pose_graph, net, frames, views, args):
    kw = dict(steps=steps, skip=10)
    if pose_graph:
        kw.update(include_vos=True, real=True, vo_func=calc_vos_safe_fc)
    sets = {"host": MF(frames, gt_dataset=frames if pose_graph else None, **kw),
            "resident": MF(views, gt_dataset=views if pose_graph else None, **kw)}
    arms = ("loop", "sequence", "sequence_resident")
    last = {arm: region(arm, net, sets, pose_graph, args)[2] for arm in arms}  # warm-up of each arm (plans, weight repack, clocks)
    agree(last["loop"], last["sequence"], pose_graph)
    agree(last["sequence"], last["sequence_resident"], pose_graph, exact=True)
    wall, split = {a: [] for a in arms}, {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            w, s, _ = region(arm, net, sets, pose_graph, args)
            wall[arm].append(w)
            split[arm].append(s)
    med = {a: statistics.median(v) for a, v in wall.items()}
    spread = {a: max(v) - min(v) for a, v in wall.items()}
    res = {"what": "whole evaluation of %d frames of %dx%d (uint8, fp16x2m, fused inference pass), %s; %d regions per arm, alternating; "
                   "sequence arms at %d frames per pass" % (len(frames), args.height, args.width, name, args.rounds, args.batch_frames),
           "wall_s": {a: [round(t, 4) for t in v] for a, v in wall.items()},
           "median_wall_s": {a: round(v, 4) for a, v in med.items()},
           "spread_s": {a: round(v, 4) for a, v in spread.items()},
           "median_split_s": {a: {k: round(statistics.median([s[k] for s in v]), 4) for k in ("forward", "host", "pgo")}
                              for a, v in split.items()},
           "frames_per_s": {a: round(len(frames) / v, 1) for a, v in med.items()},
           "arms_agree": True}
    for a in arms[1:]:
        res["%s_over_loop" % a] = round(med[a] / med["loop"], 4)
        res["%s_difference_exceeds_spread" % a] = (med["loop"] - med[a]) > max(spread["loop"], spread[a])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed regions per arm (at least 5)")
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--batch_frames", type=int, default=192)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=341)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least five regions per arm"
    assert torch.cuda.is_available(), "sequence_eval_rate.py measures the MI355X; there is no CPU fallback"
    G.set_compute_dtype("fp16x2m")
    torch.manual_seed(3)
    net = G.MapNet(G.PoseNet(G.resnet34(), droprate=0.0, pretrained=False))
    with torch.no_grad():  # random-init heads put out log-quaternions of many turns; scaled so the pose graph sees rotations below pi
        net.mapnet.fc_xyz.weight.mul_(0.01)
        net.mapnet.fc_wpqr.weight.mul_(0.01)
    net.mapnet._engine.params_touched()
    net.cuda()
    net.eval()
    net.set_input_u8(SyntheticFrames.MEAN, SyntheticFrames.STD)
    net.set_eval_fused(True)
    frames = MemFrames(args.frames, args.height, args.width)
    (views,), _ = make_resident([frames], net.mapnet._engine.device)
    lines = [json.dumps(measure(name, steps, pg, net, frames, views, args)) for name, steps, pg in CELLS]
    for ln in lines:
        print(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
