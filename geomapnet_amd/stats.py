"""Dataset pixel statistics on the device: the `mean` and `std` of the reference's `Normalize`, from uint8 frames.

The reference gets them from `stats.txt`, written by its scripts/dataset_mean.py: the training split walked through a DataLoader,
per-pixel sums accumulated in numpy.  Here the frames are summed where they are -- in HBM, after the device's own Resize when one is
asked for -- by `mn_op_frame_stats_u8` (csrc/frame_stats.h): per-channel sums and sums of squares of the bytes as 64-bit integers,
exact and independent of the order of summation.

    sums = pixel_sums(views[0], resize=256)            # a ResidentFrames view, read in place
    write_stats("stats.txt", sums)                     # the reference's file: row 0 the mean, row 1 the VARIANCE
    mean, std = read_stats("stats.txt")                # as the reference's train.py / eval.py read it: std = sqrt(row 1)
    model.set_input_u8(mean, std)

Statistics are taken over WHOLE frames: the reference's `RandomCrop(crop_size)` (dataset_mean.py:40-44, off unless crop_size > 0) is
not applied.  Plumbing only: torch tensors as containers.
"""
import ctypes as C

import numpy as np
import torch

from ._binding import MapNetHipError, ptr
from .data import resize_dims

MAX_RESIZE_FRAMES = 65535  # frames one mn_op_resize_u8[_indexed] call takes


class PixelSums:
    """Per-channel integer sums of uint8 pixels: `count` pixels (per channel), `sum` and `sumsq` numpy int64 [3].  `a + b` merges the
    sums of two datasets.  mean / var / std are float64 [3] in ToTensor's [0, 1] units: mean = sum / (255 N), var = sumsq / (255^2 N) -
    mean^2 (the population variance, as dataset_mean.py:66-70), std = sqrt(var)."""

    def __init__(self, count, sum, sumsq):
        self.count = int(count)
        self.sum = np.asarray(sum, dtype=np.int64).reshape(3).copy()
        self.sumsq = np.asarray(sumsq, dtype=np.int64).reshape(3).copy()

    def __add__(self, other):
        if not isinstance(other, PixelSums):
            return NotImplemented
        return PixelSums(self.count + other.count, self.sum + other.sum, self.sumsq + other.sumsq)

    def mean(self):
        return self.sum.astype(np.float64) / (255.0 * self.count)

    def var(self):
        return self.sumsq.astype(np.float64) / (255.0 * 255.0 * self.count) - self.mean() ** 2

    def std(self):
        return np.sqrt(np.maximum(self.var(), 0.0))

    def __repr__(self):
        return "PixelSums(count=%d, sum=%s, sumsq=%s)" % (self.count, self.sum.tolist(), self.sumsq.tolist())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None


def _check_u8(what, shape, dtype):
    if dtype != torch.uint8 or len(shape) != 3 or shape[-1] != 3:
        raise TypeError("pixel_sums: %s must be uint8 [h, w, 3] (decoded images, what set_input_u8 consumes), got %s %s"
                        % (what, dtype, list(shape)))


class _Summer:
    """the device side of one pixel_sums call: sums, flag, work and resize buffers, sized at the first chunk and kept"""

    def __init__(self, lib, dev, h, w, resize):
        self.lib, self.dev, self.h, self.w = lib, dev, h, w
        self.H, self.W = resize_dims(h, w, resize) if resize is not None else (h, w)
        if self.H < 1 or self.W < 1:
            raise ValueError("pixel_sums: resize %r gives %d x %d frames" % (resize, self.H, self.W))
        self.resize = resize is not None
        self.sums = torch.zeros(6, dtype=torch.int64, device=dev)
        self.bad = torch.zeros(2, dtype=torch.float32, device=dev)  # [0]: the resize's flag, [1]: the statistics'
        self.frames = 0
        self.work = self.rs_work = self.rs_out = None

    def _buffers(self, n):
        if self.work is None:  # n is the largest chunk: the first
            nwork = int(self.lib.op_frame_stats_work_bytes(n, self.H, self.W, 0))
            if nwork < 0:
                raise MapNetHipError(self.lib.last_error().decode())
            self.work = torch.empty(nwork // 8, dtype=torch.int64, device=self.dev)
            if self.resize:
                nrs = int(self.lib.op_resize_work_bytes(self.h, self.w, self.H, self.W))
                if nrs < 0:
                    raise MapNetHipError(self.lib.last_error().decode())
                self.rs_work = torch.empty((nrs + 3) // 4, dtype=torch.int32, device=self.dev)
                self.rs_out = torch.empty((n, self.H, self.W, 3), dtype=torch.uint8, device=self.dev)

    def add(self, frames, index, store_frames, n):
        """n images: `frames` [n, h, w, 3], or with `index` (device int32 [n]) frames index[b] of a store of `store_frames`"""
        lib, st = self.lib, _stream(self.dev)
        self._buffers(n)
        acc = 1 if self.frames else 0
        if self.resize:
            if index is None:
                lib.check(lib.op_resize_u8(ptr(frames), ptr(self.rs_out), ptr(self.rs_work), n, self.h, self.w, self.H, self.W, st))
            else:
                if self.frames:  # the flag is cleared by every call: keep what an earlier chunk raised
                    self.bad[1:2].copy_(torch.maximum(self.bad[0:1], self.bad[1:2]))
                lib.check(lib.op_resize_u8_indexed(ptr(frames), ptr(index), store_frames, ptr(self.rs_out), ptr(self.rs_work), n,
                                                   self.h, self.w, self.H, self.W, ptr(self.bad[0:1]), st))
            lib.check(lib.op_frame_stats_u8(ptr(self.rs_out), None, 0, n, self.H, self.W, ptr(self.sums), acc, 0, ptr(self.work),
                                            None, st))
        else:
            if index is not None and self.frames:
                self.bad[1:2].copy_(torch.maximum(self.bad[0:1], self.bad[1:2]))
            lib.check(lib.op_frame_stats_u8(ptr(frames), ptr(index), store_frames if index is not None else 0, n, self.H, self.W,
                                            ptr(self.sums), acc, 0, ptr(self.work), ptr(self.bad[0:1]) if index is not None else None,
                                            st))
        self.frames += n

    def result(self):
        s, bad = self.sums.cpu().numpy(), self.bad.cpu()  # the one synchronisation
        if bad.max().item() != 0:
            raise IndexError("pixel_sums: an index lies outside the frame store (the kernel counted frame 0 in its place)")
        return PixelSums(self.frames * self.H * self.W, s[:3], s[3:])


def pixel_sums(frames, index=None, resize=None, batch_frames=192, _binding=None, device=None):
    """Per-channel sums and sums of squares of uint8 frames, taken on the device -> PixelSums.

    `frames`: a device uint8 tensor [F, h, w, 3]; a `ResidentFrames` view, read in place from its slice of the store by index, with
    no copy; or any indexable dataset of (uint8 [h, w, 3] frame, pose) items on the host, staged in chunks of `batch_frames` frames
    through one pinned buffer as `ResidentFrames.build` does (onto `device`; default: the GPU of the kernel library).  `index`
    (optional, integers): the frames to take, by position in `frames`, repeats allowed; default every frame once.
    `resize` (an int or (H, W), the meaning of `set_input_resize`): every chunk goes through the device's Resize first and the
    statistics are those of the resized frames, the frames the network sees.  Whole frames are counted: the reference's
    RandomCrop(crop_size) is not applied.  Frames that are not uint8 are refused.  One host synchronisation, at the end."""
    from . import _binding as B
    from .resident import ResidentFrames
    lib = _binding if _binding is not None else B.hip()
    batch_frames = int(batch_frames)
    if batch_frames < 1:
        raise ValueError("pixel_sums: batch_frames must be at least 1, got %d" % batch_frames)
    if resize is not None:
        batch_frames = min(batch_frames, MAX_RESIZE_FRAMES)
    L = len(frames)
    if L < 1:
        raise ValueError("pixel_sums: no frames")
    if index is not None:
        index = torch.as_tensor(index).reshape(-1).cpu().long()
        if index.numel() < 1 or int(index.min()) < 0 or int(index.max()) >= L:
            raise IndexError("pixel_sums: index must be non-empty and lie in [0, %d)" % L)

    if isinstance(frames, ResidentFrames) or torch.is_tensor(frames):
        view = isinstance(frames, ResidentFrames)
        store = frames.store if view else frames
        if not torch.is_tensor(store) or store.dim() != 4 or not store.is_contiguous():
            raise TypeError("pixel_sums: frames must be a contiguous uint8 tensor [F, h, w, 3]")
        _check_u8("frames", store.shape[1:], store.dtype)
        dev = store.device
        if lib.backend_name == "hip" and dev.type != "cuda":
            raise MapNetHipError("pixel_sums: the frames are on %s; the kernels read device memory (pass a host DATASET to have it "
                                 "staged)" % dev)
        summer = _Summer(lib, dev, int(store.shape[1]), int(store.shape[2]), resize)
        if view or index is not None:  # by index, in place
            base = frames.base if view else 0
            idx = (base + (index if index is not None else torch.arange(L))).to(device=dev, dtype=torch.int32)
            for s in range(0, idx.numel(), batch_frames):
                part = idx[s:s + batch_frames]
                summer.add(store, part, int(store.shape[0]), int(part.numel()))
        else:
            for s in range(0, L, batch_frames):
                part = store[s:s + batch_frames]
                summer.add(part, None, 0, int(part.shape[0]))
        return summer.result()

    # a host dataset: chunks through one pinned staging buffer
    dev = torch.device(device if device is not None else ("cuda" if lib.backend_name == "hip" else "cpu"))
    order = index.tolist() if index is not None else range(L)
    first, _ = frames[order[0]]
    first = torch.as_tensor(first)
    _check_u8("the dataset's frames", first.shape, first.dtype)
    shape = tuple(first.shape)
    summer = _Summer(lib, dev, shape[0], shape[1], resize)
    chunk = min(batch_frames, len(order))
    stage = torch.empty((chunk,) + shape, dtype=torch.uint8, pin_memory=dev.type == "cuda")
    on_dev = torch.empty((chunk,) + shape, dtype=torch.uint8, device=dev)
    fill = 0
    for k, i in enumerate(order):
        frame = torch.as_tensor(frames[i][0])
        if tuple(frame.shape) != shape or frame.dtype != torch.uint8:
            raise TypeError("pixel_sums: frame %d is %s %s, the first one uint8 %s" % (i, frame.dtype, list(frame.shape), list(shape)))
        stage[fill].copy_(frame)
        fill += 1
        if fill == chunk or k == len(order) - 1:
            on_dev[:fill].copy_(stage[:fill], non_blocking=True)
            summer.add(on_dev, None, 0, fill)
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()  # one staging buffer: refilled only after its copy
            fill = 0
    return summer.result()


def write_stats(path, sums):
    """the reference's stats.txt (dataset_mean.py:66-73): np.savetxt of [mean; VARIANCE], '%8.7f'"""
    np.savetxt(path, np.vstack((sums.mean(), sums.var())), fmt="%8.7f")
    return path


def read_stats(path):
    """-> (mean, std) float64 [3] as the reference's train.py:127 / eval.py:101 read stats.txt: std = sqrt(row 1)"""
    stats = np.loadtxt(path)
    if stats.shape != (2, 3):
        raise ValueError("read_stats: %s holds %s values, expected 2 rows (mean, variance) of 3" % (path, list(stats.shape)))
    return stats[0], np.sqrt(stats[1])
