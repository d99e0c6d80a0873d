"""What the dataset pixel statistics (csrc/frame_stats.h, geomapnet_amd.pixel_sums) cost on the MI355X, the store resident:
  1 000 frames of 256x341                 one mn_op_frame_stats_u8 call over the store, and pixel_sums over a ResidentFrames view
  1 000 frames of 480x640                 the same
  1 000 frames of 480x640, Resize(256)    pixel_sums(view, resize=256): chunks of --batch_frames through mn_op_resize_u8_indexed
HIP events around each call, median of --reps; each against the byte floor of the same read (the frames once; with Resize the source
once plus the resized frames written and read once) at the HBM rate a copy reaches (6.29 TB/s, MI355X_MICROARCH), and against the host
path on the same frames: the reference's scripts/dataset_mean.py loop restated in numpy (ToTensor's fp32 x / 255, batches of 8
summed, squares, float64 accumulators; PIL's resize first in the Resize case), timed on the first --host_frames frames and scaled to
all of them.  Every device result is checked against torch's int64 sums of the same bytes.
usage: python tools/frame_stats_rate.py [--frames 1000] [--reps 9] [--host_frames 96] [--batch_frames 192]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geomapnet_amd import ResidentFrames, _binding, pixel_sums  # noqa: E402
from geomapnet_amd._binding import ptr  # noqa: E402
from geomapnet_amd.data import resize_dims  # noqa: E402

HBM_COPY_BPS = 6.29e12  # measured float4 copy


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return us


def device_sums(x):
    """int64 [6] of a device uint8 tensor [n, h, w, 3], by torch, in chunks"""
    s = torch.zeros(6, dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], 50):
        v = x[i:i + 50].reshape(-1, 3).to(torch.int64)
        s[:3] += v.sum(0)
        s[3:] += (v * v).sum(0)
    return s.cpu().numpy()


def host_path(u8, size):
    """the reference's loop on host frames [n, h, w, 3] -> seconds"""
    t0 = time.perf_counter()
    if size is not None:
        from PIL import Image
        H, W = resize_dims(u8.shape[1], u8.shape[2], size)
        u8 = np.stack([np.asarray(Image.fromarray(f).resize((W, H), Image.BILINEAR)) for f in u8])
    n, h, w, _ = u8.shape
    acc, sq_acc = np.zeros((3, h, w)), np.zeros((3, h, w))
    for i in range(0, n, 8):
        imgs = np.transpose(u8[i:i + 8], (0, 3, 1, 2)).astype(np.float32) / np.float32(255)
        acc += np.sum(imgs, axis=0)
        sq_acc += np.sum(imgs ** 2, axis=0)
    mean = acc.reshape(3, -1).sum(1) / (n * h * w)
    var = sq_acc.reshape(3, -1).sum(1) / (n * h * w) - mean ** 2
    assert np.isfinite(var).all()
    return time.perf_counter() - t0


def case(lib, args, h, w, size):
    n = args.frames
    gen = torch.Generator(device="cuda").manual_seed(h + w)
    store = torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.uint8, device="cuda")
    view = ResidentFrames(store, 0, n, torch.zeros(n, 6))
    src_bytes = store.numel()
    what = "%d frames of %dx%d" % (n, h, w)
    rows = []
    if size is None:
        want = device_sums(store)
        floor = src_bytes
        sums = torch.zeros(6, dtype=torch.int64, device="cuda")
        work = torch.empty(int(lib.op_frame_stats_work_bytes(n, h, w, 0)) // 8, dtype=torch.int64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def op():
            lib.check(lib.op_frame_stats_u8(ptr(store), None, 0, n, h, w, ptr(sums), 0, 0, ptr(work), None, st))

        rows.append(("mn_op_frame_stats_u8, one call, %d workgroups" % (work.numel() // 6), timed(op, args.reps)))
        assert np.array_equal(sums.cpu().numpy(), want)
    else:
        H, W = resize_dims(h, w, size)
        what += ", Resize(%d) -> %dx%d" % (size, H, W)
        floor = src_bytes + 2 * n * H * W * 3
        want = None
    got = []

    def whole():
        got.append(pixel_sums(view, resize=size, batch_frames=args.batch_frames))  # (ends in its one read-back of the sums)

    rows.append(("pixel_sums(view%s), chunks of %d, with the read-back of the sums" % ("" if size is None else ", resize=%d" % size,
                                                                                         args.batch_frames), timed(whole, args.reps)))
    if want is not None:
        assert np.array_equal(np.concatenate([got[-1].sum, got[-1].sumsq]), want)
    else:  # against torch's sums of frames the device resized on its own
        out = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda")
        rs_work = torch.empty(int(lib.op_resize_work_bytes(h, w, H, W)), dtype=torch.uint8, device="cuda")
        for s in range(0, n, 192):
            m = min(192, n - s)
            lib.check(lib.op_resize_u8(ptr(store[s:]), ptr(out[s:]), ptr(rs_work), m, h, w, H, W,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert np.array_equal(np.concatenate([got[-1].sum, got[-1].sumsq]), device_sums(out))
    assert all(np.array_equal(g.sum, got[0].sum) and np.array_equal(g.sumsq, got[0].sumsq) for g in got)  # run to run: the same integers
    nh = min(args.host_frames, n)
    host_path(store[:8].cpu().numpy(), size)  # (warm-up: numpy's and PIL's first use)
    host_s = host_path(store[:nh].cpu().numpy(), size) * n / nh
    floor_us = 1e6 * floor / HBM_COPY_BPS
    for name, us in rows:
        med = statistics.median(us)
        print(json.dumps({"what": what, "call": name, "us_median": round(med, 1), "us_min": round(min(us), 1),
                          "us_max": round(max(us), 1), "reps": len(us), "floor_bytes": floor, "floor_us_at_6.29TBps": round(floor_us, 1),
                          "fraction_of_floor": round(floor_us / med, 3), "GBps_of_floor": round(floor / med / 1e3, 1),
                          "host_numpy_s_scaled_from_%d_frames" % nh: round(host_s, 3), "host_over_device": round(host_s * 1e6 / med, 1)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host_frames", type=int, default=96)
    ap.add_argument("--batch_frames", type=int, default=192)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frame_stats_rate.py measures the MI355X; there is no CPU fallback"
    lib = _binding.hip()
    case(lib, args, 256, 341, None)
    case(lib, args, 480, 640, None)
    case(lib, args, 480, 640, 256)


if __name__ == "__main__":
    main()
