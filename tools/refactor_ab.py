"""A/B material for host-only refactors of the library: run it once per build (MN_LIB names the library, as for
tools/conv_bench.py; unset = this tree's) and compare the two outputs.

  python tools/refactor_ab.py bits [--dtype D]
      MN_DETERMINISTIC=1, 2 windows x T=3 at 64x85, per dtype: one MapNet training step (clip 5.0), one eval forward pass on the
      stepped weights (fp16x2 / fp16x2m: a second one with the fused pass), fp32 / fp16: one input_grad call with saliency.  One line
      per (dtype, quantity): the first 16 hex digits of the sha256 of its bytes.  Equal lines = the same kernels got the same
      arguments in every launch the small shape reaches.
  python tools/refactor_ab.py steps --dtype D
      the benchmark's shape (64 windows x T=3, 256x341; --windows halves it where a mode does not fit): two training steps, one
      eval forward pass, for the h2 dtypes one fused eval forward pass.  Prints "ok"; it exists to have a kernel trace wrapped
      around it, whose (kernel, grid, workgroup) census shows the choices taken at the workload's tile counts."""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geomapnet_amd as G  # noqa: E402

DTYPES = ("fp32", "fp16", "fp32x3", "fp16x2", "fp16x2m", "fp16x2q")
FUSED = ("fp16x2", "fp16x2m")
INPUT_GRAD = ("fp32", "fp16")
DEV = "cuda"
BITS_SHAPE = (2, 64, 85)  # windows, H, W


def setup(dtype, windows, H, W):
    G.set_compute_dtype(dtype)
    torch.manual_seed(3)
    net = G.MapNet(G.PoseNet(G.resnet34(), droprate=0.0, pretrained=False))
    crit = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True)
    net.to(DEV)
    crit.to(DEV)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [crit.sax, crit.saq]}, {"params": [crit.srx, crit.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    x = torch.randn(windows, 3, 3, H, W).to(DEV)
    t = (torch.randn(windows, 3, 6) * 0.5).to(DEV)
    return net, crit, opt, x, t


def train_and_eval(dtype, net, crit, opt, x, t, steps, report):
    net.train()
    for _ in range(steps):
        loss, poses = G.step_feedfwd(x, net, True, t, crit, opt, True, max_grad_norm=5.0)
    eng = net.mapnet._engine
    report("loss", torch.tensor([loss]))
    report("poses", poses)
    report("params", eng.params)
    report("grads", eng.grads())
    report("opt_state", eng.opt_state[eng.n_params:])
    net.eval()
    report("eval_poses", net(x))
    if dtype in FUSED:
        net.set_eval_fused(True)
        report("eval_poses_fused", net(x))
        net.set_eval_fused(False)


def bits(args):
    os.environ["MN_DETERMINISTIC"] = "1"  # (read when a plan is created)
    for dtype in [args.dtype] if args.dtype else DTYPES:
        def report(name, tensor):
            digest = hashlib.sha256(tensor.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
            print("%-8s %-17s %s" % (dtype, name, digest), flush=True)
        net, crit, opt, x, t = setup(dtype, *BITS_SHAPE)
        train_and_eval(dtype, net, crit, opt, x, t, 1, report)
        if dtype in INPUT_GRAD:
            gx, poses, maps = net.mapnet._input_grad(x.flatten(0, 1), None, True)
            report("input_grad_gx", gx)
            report("input_grad_poses", poses)
            report("saliency", maps)


def steps(args):
    net, crit, opt, x, t = setup(args.dtype, args.windows, 256, 341)
    train_and_eval(args.dtype, net, crit, opt, x, t, 2, lambda name, tensor: None)
    torch.cuda.synchronize()
    print("ok")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("bits")
    b.add_argument("--dtype", choices=DTYPES)
    b.set_defaults(fn=bits)
    s = sub.add_parser("steps")
    s.add_argument("--dtype", choices=DTYPES, required=True)
    s.add_argument("--windows", type=int, default=64)
    s.set_defaults(fn=steps)
    args = ap.parse_args()
    args.fn(args)
