"""Device-resident frame store: the frames of whole sequences uploaded once, every batch gathered by index in HBM.

The reference assembles a batch on the host: DataLoader workers run `MF.__getitem__` (a `torch.stack` of `steps` frames,
/root/reference/dataset_loaders/composite.py:77-83), `default_collate` stacks the windows (common/train.py:180-188) and the
result crosses PCIe.  Every frame is copied once per window it appears in, i.e. `steps` times per epoch.  The sequences the
reference trains on are small next to HBM (a 7Scenes scene: at most 6.4 GB of raw 480x640 uint8 frames), so here they can live on
the device:

    views = ResidentFrames.build([train_frames, val_frames], device)      # ONE device tensor, one view per dataset
    train_set = MF(views[0], steps=3, skip=10)                            # a view is itself a frame dataset
    for frames, target in ResidentLoader(train_set, batch_size=64, shuffle=True, device=device):
        loss, _ = step_feedfwd(frames, model, True, target, criterion, optim, True)   # frames: IndexedFrames

What crosses PCIe per step is the index vector (4 bytes per frame) and the pose targets; the library gathers the frames at the head
of the pass (include/mapnet_hip.h mn_set_input_index).  Plumbing only: torch tensors as containers.
"""
import copy

import numpy as np
import torch

from ._binding import MapNetHipError
from .feed import DeviceFeed


def free_memory(device):
    """bytes free on `device` (torch.cuda.mem_get_info), or None where there is nothing to ask (a CPU device)"""
    device = torch.device(device)
    if device.type != "cuda":
        return None
    return int(torch.cuda.mem_get_info(device)[0])


class ResidentFrames(torch.utils.data.Dataset):
    """One dataset's slice of a device-resident frame store: frames [base, base + len) of `store`.  Indexable like the dataset it
    was built from -- (frame, pose), the frame a device tensor -- so MF / MFOnline take it as their frame dataset; `poses` (CPU
    [L, 6]) and `gt_idx` are what `index_item` reads instead of touching a frame."""

    def __init__(self, store, base, length, poses, gt_idx=None):
        self.store, self.base, self.length, self.poses, self.gt_idx = store, int(base), int(length), poses, gt_idx

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < self.length:
            raise IndexError(i)
        return self.store[self.base + i], self.poses[i]

    def index_item(self, i):
        """-> (store index of frame i, pose): the PoseNet sample without its frame"""
        i = int(i)
        if not 0 <= i < self.length:
            raise IndexError(i)
        return torch.tensor(self.base + i, dtype=torch.int32), self.poses[i]

    CHUNK_BYTES = 64 << 20  # the pinned staging buffer

    @staticmethod
    def build(datasets, device):
        """Uploads every frame of `datasets` (indexable, (frame, pose) items) into ONE tensor on `device`, in chunks through one
        pinned staging buffer; returns one view per dataset.  All frames share dtype and size.  The store must fit the device's
        free memory as reported before the upload: there is no streaming fallback."""
        device = torch.device(device)
        datasets = list(datasets)
        if not datasets or any(len(d) < 1 for d in datasets):
            raise ValueError("ResidentFrames.build: needs at least one dataset, each with at least one frame")
        first, _ = datasets[0][0]
        shape, dtype = tuple(first.shape), first.dtype
        total = sum(len(d) for d in datasets)
        frame_bytes = int(np.prod(shape)) * first.element_size()
        nbytes = total * frame_bytes
        free = free_memory(device)
        if free is not None and nbytes > free:
            raise MapNetHipError("ResidentFrames.build: the store needs %d bytes (%d frames of %d bytes) and %s reports %d bytes free; "
                                 "frames stay on the host loader, nothing was uploaded" % (nbytes, total, frame_bytes, device, free))
        store = torch.empty((total,) + shape, dtype=dtype, device=device)
        chunk = max(1, min(total, ResidentFrames.CHUNK_BYTES // frame_bytes))
        stage = torch.empty((chunk,) + shape, dtype=dtype, pin_memory=device.type == "cuda")
        views, pos = [], 0
        for d in datasets:
            poses, base, fill = [], pos, 0
            for i in range(len(d)):
                frame, pose = d[i]
                if tuple(frame.shape) != shape or frame.dtype != dtype:
                    raise ValueError("ResidentFrames.build: frame %d of dataset %d is %s %s, the store holds %s %s"
                                     % (i, len(views), frame.dtype, list(frame.shape), dtype, list(shape)))
                stage[fill].copy_(frame)
                poses.append(torch.as_tensor(pose))
                fill += 1
                if fill == chunk or i == len(d) - 1:
                    store[pos:pos + fill].copy_(stage[:fill], non_blocking=True)
                    if device.type == "cuda":
                        torch.cuda.current_stream(device).synchronize()  # one staging buffer: refilled only after its copy
                    pos, fill = pos + fill, 0
            views.append(ResidentFrames(store, base, len(d), torch.stack(poses, dim=0), getattr(d, "gt_idx", None)))
        return views


class IndexedFrames:
    """`store[index]` without the gather: what a model, `step_feedfwd`, `input_gradient` and `saliency` accept in place of an image
    tensor.  store: [F, 3, H, W] fp32 or [F, h, w, 3] uint8 frames on the model's device; index: int32 / int64 [N] (PoseNet) or
    [N, T] (MapNet).  An index on the host is range-checked here and uploaded; one already on the store's device is used as it
    is (the kernels map an index outside the store to frame 0 and flag it: Engine.input_index_bad)."""

    def __init__(self, store, index):
        if not torch.is_tensor(store) or store.dim() != 4 or not store.is_contiguous():
            raise ValueError("IndexedFrames: store must be a contiguous tensor of frames [F, 3, H, W] or [F, h, w, 3]")
        index = torch.as_tensor(index)
        if index.dtype not in (torch.int32, torch.int64) or index.dim() not in (1, 2) or index.numel() < 1:
            raise ValueError("IndexedFrames: index must be int32 or int64, [N] or [N, T]")
        if index.device.type == "cpu":  # built on the host: checked before anything is uploaded or launched
            lo, hi = int(index.min()), int(index.max())
            if lo < 0 or hi >= store.shape[0]:
                raise ValueError("IndexedFrames: index range [%d, %d] leaves the store's %d frames" % (lo, hi, store.shape[0]))
            index = index.to(device=store.device, dtype=torch.int32, non_blocking=True)
        elif index.device != store.device:
            raise ValueError("IndexedFrames: index on %s but store on %s" % (index.device, store.device))
        self.store = store
        self.index = index.to(torch.int32).contiguous()

    # -- the tensor surface the input path reads: everything describes store[index]
    @property
    def shape(self):
        return torch.Size(tuple(self.index.shape) + tuple(self.store.shape[1:]))

    def size(self, *a):
        return self.shape if not a else self.shape[a[0]]

    def dim(self):
        return len(self.shape)

    @property
    def dtype(self):
        return self.store.dtype

    @property
    def device(self):
        return self.store.device

    @property
    def is_cuda(self):
        return self.store.is_cuda

    # the few tensor methods the input path calls (PoseNet.forward, step_feedfwd): none of them copies or converts a frame
    def detach(self):
        return self

    def contiguous(self):
        return self

    def float(self):
        if self.store.dtype != torch.float32:  # (no silent no-op: the store is what the kernels will read)
            raise TypeError("IndexedFrames over a %s store cannot become fp32 frames; uint8 frames need model.set_input_u8"
                            % self.store.dtype)
        return self

    def __getattr__(self, name):
        raise AttributeError("IndexedFrames stands for store[index] on the models' input path only and has no %r; "
                             "use .gather() for the tensor" % name)

    def to(self, device, **kw):
        if torch.device(device).type != self.device.type:  # (never a copy: the point is that the frames stay where they are)
            raise RuntimeError("IndexedFrames live on the store's device (%s); asked for %s" % (self.device, device))
        return self

    def reshape(self, *shape):
        """only the collapse MapNet.forward does: [N, T, ...] -> [N*T, ...]"""
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        if tuple(shape[1:]) != tuple(self.store.shape[1:]) or shape[0] not in (-1, self.index.numel()):
            raise ValueError("IndexedFrames.reshape: only (-1, *frame) is supported")
        out = IndexedFrames.__new__(IndexedFrames)
        out.store, out.index = self.store, self.index.reshape(-1)
        return out

    def gather(self):
        """the tensor this stands for (tests, tools): store[index]"""
        return self.store[self.index.long()]


class _PosesOnly(torch.utils.data.Dataset):
    """a ground-truth dataset as MF reads it (`real=True`: poses, never frames), without its frames"""

    def __init__(self, dataset):
        poses = getattr(dataset, "poses", None)
        self.poses = torch.as_tensor(poses) if poses is not None else torch.stack([torch.as_tensor(dataset[i][1])
                                                                                   for i in range(len(dataset))], dim=0)

    def __len__(self):
        return self.poses.shape[0]

    def __getitem__(self, i):
        return torch.empty(0), self.poses[int(i)]


def make_resident(window_datasets, device):
    """-> (copies of `window_datasets` over resident views, the store).  Every frame dataset the windows take frames from (MF.dset,
    MFOnline's two MFs, or a frame dataset itself for PoseNet) is uploaded once into one store; a dataset used twice stays one.  A
    ground-truth dataset (MF.gt_dset) supplies poses only: unless it is also a frame dataset, its frames are not uploaded."""
    frames, order = {}, []

    def note(d):
        if d is not None and id(d) not in frames:
            frames[id(d)] = None
            order.append(d)

    def walk(w, fn):
        if hasattr(w, "train_set") and hasattr(w, "val_set"):  # MFOnline
            w = copy.copy(w)
            w.train_set, w.val_set = walk(w.train_set, fn), walk(w.val_set, fn)
            return w
        if hasattr(w, "dset"):  # MF
            w = copy.copy(w)
            w.dset, w.gt_dset = fn(w.dset, False), fn(w.gt_dset, True)
            return w
        return fn(w, False)

    def collect(d, poses_only):
        if not poses_only:
            note(d)
        return d

    def resident(d, poses_only):
        if d is None:
            return None
        if id(d) not in frames:  # a ground-truth dataset no window takes frames from
            frames[id(d)] = _PosesOnly(d)
        return frames[id(d)]

    for w in window_datasets:
        walk(w, collect)
    views = ResidentFrames.build(order, device)
    for d, v in zip(order, views):
        frames[id(d)] = v
    out = [walk(w, resident) for w in window_datasets]
    return out, views[0].store


class _IndexItems(torch.utils.data.Dataset):
    """the `index_item` view of a window dataset: what ResidentLoader's DataLoader iterates"""

    def __init__(self, dataset):
        if not hasattr(dataset, "index_item"):
            raise TypeError("ResidentLoader needs a dataset with index_item (MF / MFOnline over ResidentFrames views, or a view)")
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, i):
        return self.dataset.index_item(i)


def _store_of(dataset):
    for name in ("store", "dset", "val_set", "train_set"):
        d = getattr(dataset, name, None)
        if torch.is_tensor(d):
            return d
        if d is not None:
            return _store_of(d)
    raise TypeError("ResidentLoader: %r is not built over ResidentFrames views" % type(dataset).__name__)


class _Checked:
    """the host range check of every index batch, before DeviceFeed uploads it"""

    def __init__(self, loader, frames):
        self.loader, self.frames = loader, frames

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for index, target in self.loader:
            lo, hi = int(index.min()), int(index.max())
            if lo < 0 or hi >= self.frames:
                raise ValueError("ResidentLoader: index range [%d, %d] leaves the store's %d frames" % (lo, hi, self.frames))
            yield index, target


class ResidentLoader:
    """The reference's DataLoader (common/train.py:180-188) over the `index_item` view of `window_dataset`: the same sampler, batch
    size and collate function, so under a given torch seed the batch order is by construction the host loader's; no workers -- an
    item is a few integers and poses.  Index and target batches go through DeviceFeed's race-free rotation; yields
    (IndexedFrames, target)."""

    def __init__(self, window_dataset, batch_size=1, shuffle=False, sampler=None, drop_last=False, device=None):
        from .trainer import safe_collate
        self.store = _store_of(window_dataset)
        if device is not None:  # where the consumer runs: it must be where the frames are
            device = torch.device(device)
            if device.type != self.store.device.type or device.index not in (None, self.store.device.index):
                raise ValueError("ResidentLoader: the store is on %s, the batches are wanted on %s" % (self.store.device, device))
        self.loader = torch.utils.data.DataLoader(_IndexItems(window_dataset), batch_size=batch_size, shuffle=shuffle, sampler=sampler,
                                                  num_workers=0, collate_fn=safe_collate, drop_last=drop_last,
                                                  pin_memory=self.store.is_cuda)
        self._feed = DeviceFeed(_Checked(self.loader, int(self.store.shape[0])), self.store.device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for index, target in self._feed:
            frames = IndexedFrames.__new__(IndexedFrames)  # (range-checked above; already int32 on the store's device)
            frames.store, frames.index = self.store, index.to(device=self.store.device, dtype=torch.int32).contiguous()
            yield frames, target
