"""Backend-agnostic checks of the pixel statistics (csrc/frame_stats.h, mn_op_frame_stats_u8, geomapnet_amd/stats.py): each takes a
Binding (`lib`) and a torch device, so the CPU suite runs them on the SIMT-emulator build and the GPU suite on libmapnet_hip.so.
The sums of bytes are integers: every operator and `pixel_sums` comparison is exact equality with numpy's int64 sums."""
import ctypes as C

import numpy as np
import torch

import checks
from geomapnet_amd._binding import ptr

GUARD = 64  # bytes of 255 on either side of the input
SHAPES = ((1, 1, 1), (2, 9, 11), (3, 33, 47), (1, 32, 40), (5, 40, 53))  # (3, 33, 47): 4 653 bytes a frame, no multiple of 16 or 48
OFFSETS = (0, 1, 5, 16)  # where the data starts in its allocation
POISON = -0x123456789ABCDEF  # what `sums` holds before a call that must overwrite it


def frames(n, h, w, seed, lo=0, hi=256):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, (n, h, w, 3), generator=gen, dtype=torch.uint8)


def np_sums(u8):
    """int64 [6]: per-channel sum | per-channel sum of squares"""
    x = (u8.numpy() if torch.is_tensor(u8) else np.asarray(u8)).reshape(-1, 3).astype(np.int64)
    return np.concatenate([x.sum(0), (x * x).sum(0)])


def work_bytes(lib, images, H, W, blocks=0):
    n = int(lib.op_frame_stats_work_bytes(images, H, W, blocks))
    assert n > 0 and n % 48 == 0, n
    return n


def run_op(lib, dev, u8, index=None, offset=0, blocks=0, accumulate=0, sums=None, want_bad=False):
    """mn_op_frame_stats_u8 over `u8` [F, H, W, 3] placed `offset` bytes into an allocation whose other bytes are 255 -> int64 [6]
    (and the flag, with an index).  Checks that the input, the guards and the bytes around `sums` and `work` are left as they were."""
    F, H, W, _ = u8.shape
    n = u8.numel()
    buf = torch.full((GUARD + offset + n + GUARD,), 255, dtype=torch.uint8)
    buf[GUARD + offset:GUARD + offset + n] = u8.reshape(-1)
    d = buf.to(dev)
    x = d[GUARD + offset:GUARD + offset + n]
    images = F if index is None else len(index)
    idx = None if index is None else torch.as_tensor(index, dtype=torch.int32).to(dev)
    nwork = work_bytes(lib, images, H, W, blocks)
    wbuf = torch.full((nwork // 8 + 2,), -1, dtype=torch.int64, device=dev)
    sbuf = torch.full((8,), -1, dtype=torch.int64, device=dev)
    if sums is not None:
        sbuf[1:7] = torch.as_tensor(np.asarray(sums, dtype=np.int64)).to(dev)
    else:
        sbuf[1:7] = POISON
    bad = torch.full((3,), 7.0, dtype=torch.float32, device=dev)
    lib.check(lib.op_frame_stats_u8(ptr(x), ptr(idx), F if index is not None else 0, images, H, W, ptr(sbuf[1:7]), accumulate, blocks,
                                    ptr(wbuf[1:-1]), ptr(bad[1:2]) if index is not None else None, None))
    checks.dev_sync(dev)
    assert torch.equal(d.cpu(), buf), "the kernel wrote to its input or the guards"
    s, wk, b = sbuf.cpu(), wbuf.cpu(), bad.cpu()
    assert s[0] == -1 and s[7] == -1 and wk[0] == -1 and wk[-1] == -1, "the kernel wrote around sums or work"
    assert b[0] == 7.0 and b[2] == 7.0
    if index is None:
        assert b[1] == 7.0  # no index: the flag is not touched
    else:
        assert b[1] == (1.0 if want_bad else 0.0), b.tolist()
    return s[1:7].numpy().copy()


def check_shapes(lib, dev, shapes=SHAPES, offsets=OFFSETS):
    for k, (n, h, w) in enumerate(shapes):
        u8 = frames(n, h, w, seed=100 + k)
        want = np_sums(u8)
        for off in offsets:
            got = run_op(lib, dev, u8, offset=off)
            assert np.array_equal(got, want), ((n, h, w), off, got, want)


def check_indexed(lib, dev):
    u8 = frames(6, 33, 47, seed=120)
    for off in (0, 5):
        index = [4, 1, 4, 0, 5, 1, 1]  # a subset, repeats, shuffled
        got = run_op(lib, dev, u8, index=index, offset=off)
        assert np.array_equal(got, np_sums(u8[index]))
        bad_index = [2, 6, 3]  # 6 is outside the store of 6: counts frame 0, raises the flag
        got = run_op(lib, dev, u8, index=bad_index, offset=off, want_bad=True)
        assert np.array_equal(got, np_sums(u8[[2, 0, 3]]))
        got = run_op(lib, dev, u8, index=[-1], offset=off, want_bad=True)
        assert np.array_equal(got, np_sums(u8[[0]]))


def check_accumulate(lib, dev):
    u8 = frames(5, 40, 53, seed=130)
    whole = run_op(lib, dev, u8)
    assert np.array_equal(whole, np_sums(u8))
    first = run_op(lib, dev, u8[:2])  # accumulate = 0 over a poisoned sums
    both = run_op(lib, dev, u8[2:], accumulate=1, sums=first)
    assert np.array_equal(both, whole)
    again = run_op(lib, dev, u8[2:], accumulate=0, sums=first)
    assert np.array_equal(again, np_sums(u8[2:]))


def check_blocks(lib, dev):
    u8 = frames(5, 40, 53, seed=140)
    want = np_sums(u8)
    assert work_bytes(lib, 5, 40, 53, 1) == 48 and work_bytes(lib, 5, 40, 53, 3) == 3 * 48
    assert work_bytes(lib, 5, 40, 53, 1000) == 5 * 48  # never more workgroups than units: one unit per frame of 6 360 bytes
    for blocks in (1, 3, 0, 1000):
        got = run_op(lib, dev, u8, blocks=blocks)
        assert np.array_equal(got, want), (blocks, got, want)
    big = frames(2, 64, 130, seed=141)  # 24 960 bytes a frame: three units each, so workgroups start and stop inside a frame
    for blocks in (1, 4, 5, 0):
        for off in (0, 5):
            assert np.array_equal(run_op(lib, dev, big, blocks=blocks, offset=off), np_sums(big)), (blocks, off)


def check_saturated(lib, dev, n=2, h=256, w=341, blocks=0):
    """all 255: the sums of squares pass 2^32 (2 x 256 x 341: 1.135e10), so a 32-bit stage anywhere past the lanes shows up"""
    u8 = torch.full((n, h, w, 3), 255, dtype=torch.uint8)
    px = n * h * w
    want = np.array([255 * px] * 3 + [255 * 255 * px] * 3, dtype=np.int64)
    assert want[3] > 2 ** 32
    got = run_op(lib, dev, u8, blocks=blocks)
    assert np.array_equal(got, want), (got, want)


def check_errors(lib, dev):
    u8 = frames(2, 4, 4, seed=1).to(dev)
    sums = torch.zeros(8, dtype=torch.int64, device=dev)
    work = torch.zeros(64, dtype=torch.int64, device=dev)
    idx = torch.zeros(4, dtype=torch.int32, device=dev)
    bytes_ = torch.zeros(64, dtype=torch.uint8, device=dev)

    def refused(*a):
        assert lib.op_frame_stats_u8(*a) != 0
        msg = lib.last_error().decode()
        assert "mn_op_frame_stats_u8" in msg, msg
        return msg

    ok = (ptr(u8), None, 0, 2, 4, 4, ptr(sums), 0, 0, ptr(work), None, None)
    for i in (0, 6, 9):  # frames, sums, work
        refused(*(ok[:i] + (None,) + ok[i + 1:]))
    for i in (3, 4, 5):  # images, H, W
        for v in (0, -2):
            assert "positive" in refused(*(ok[:i] + (v,) + ok[i + 1:]))
    assert "aligned" in refused(*(ok[:6] + (C.c_void_p(sums.data_ptr() + 4),) + ok[7:]))
    assert "aligned" in refused(*(ok[:9] + (C.c_void_p(work.data_ptr() + 4),) + ok[10:]))
    assert "index" in refused(ptr(u8), C.c_void_p(bytes_.data_ptr() + 1), 2, 2, 4, 4, ptr(sums), 0, 0, ptr(work), None, None)
    assert "store_frames" in refused(ptr(u8), ptr(idx), 0, 2, 4, 4, ptr(sums), 0, 0, ptr(work), None, None)
    refused(*(ok[:8] + (-1,) + ok[9:]))
    for a in ((0, 4, 4, 0), (1, 0, 4, 0), (1, 4, -1, 0), (1, 4, 4, -1)):
        assert lib.op_frame_stats_work_bytes(*a) == -1
        assert "mn_op_frame_stats_work_bytes" in lib.last_error().decode()
    checks.dev_sync(dev)
    assert not sums.cpu().any() and not work.cpu().any()  # nothing was launched


# ---- geomapnet_amd.stats ---------------------------------------------------------------------------------------------------------
class HostFrames(torch.utils.data.Dataset):
    """a host dataset of (uint8 frame, pose) items"""

    def __init__(self, u8):
        self.u8 = u8

    def __len__(self):
        return self.u8.shape[0]

    def __getitem__(self, i):
        return self.u8[int(i)], torch.zeros(6)


def same(a, b):
    return a.count == b.count and np.array_equal(a.sum, b.sum) and np.array_equal(a.sumsq, b.sumsq)


def expect(u8):
    from geomapnet_amd.stats import PixelSums
    s = np_sums(u8)
    x = u8.numpy() if torch.is_tensor(u8) else u8
    return PixelSums(x.size // 3, s[:3], s[3:])


def check_sources(lib, dev):
    from geomapnet_amd import ResidentFrames, pixel_sums
    a, b = frames(3, 33, 47, seed=200), frames(7, 33, 47, seed=201)
    views = ResidentFrames.build([HostFrames(a), HostFrames(b)], dev)
    assert views[1].base == 3
    want = expect(b)
    assert want.sum.dtype == np.int64 and want.count == 7 * 33 * 47
    got = [pixel_sums(views[1], _binding=lib), pixel_sums(b.to(dev), _binding=lib), pixel_sums(HostFrames(b), _binding=lib)]
    for g in got:
        assert g.sum.dtype == np.int64 and g.sumsq.dtype == np.int64
        assert same(g, want), (g, want)
    # batch_frames: chunks of 1 and of 4 over 7 frames, every source
    for src in (views[1], b.to(dev), HostFrames(b)):
        assert same(pixel_sums(src, batch_frames=1, _binding=lib), want)
        assert same(pixel_sums(src, batch_frames=4, _binding=lib), want)
    # an explicit index into a tensor
    assert same(pixel_sums(b.to(dev), index=[6, 0, 0], _binding=lib), expect(b[[6, 0, 0]]))
    # __add__: two views = the concatenation
    total = pixel_sums(views[0], _binding=lib) + pixel_sums(views[1], _binding=lib)
    assert same(total, expect(torch.cat([a, b])))
    m, v = total.mean(), total.var()
    x = torch.cat([a, b]).numpy().reshape(-1, 3).astype(np.float64) / 255
    assert m.dtype == np.float64 and np.allclose(m, x.mean(0), rtol=0, atol=1e-14)
    assert np.allclose(v, x.var(0), rtol=0, atol=1e-13) and np.allclose(total.std(), x.std(0), rtol=0, atol=1e-13)
    # refusals
    for bad_frames in (b.to(dev).float(), HostFrames(b.float())):
        try:
            pixel_sums(bad_frames, _binding=lib)
            raise AssertionError("non-uint8 frames must be refused")
        except (TypeError, ValueError) as e:
            assert "uint8" in str(e), str(e)


def check_resize(lib, dev):
    import resize_ref
    from geomapnet_amd import ResidentFrames, pixel_sums
    from geomapnet_amd.data import resize_dims
    u8 = frames(5, 33, 47, seed=210)
    views = ResidentFrames.build([HostFrames(frames(2, 33, 47, seed=211)), HostFrames(u8)], dev)
    for size in (20, 40, (18, 50)):  # shrinking, enlarging, a pair
        H, W = resize_dims(33, 47, size)
        want = expect(resize_ref.resize(u8.numpy(), H, W))
        assert want.count == 5 * H * W
        for src in (views[1], u8.to(dev), HostFrames(u8)):  # the resident indexed route and the plain route
            for bf in (192, 2):
                got = pixel_sums(src, resize=size, batch_frames=bf, _binding=lib)
                assert same(got, want), (size, type(src).__name__, bf, got, want)


def reference_stats(u8, batch=8):
    """the arithmetic of the reference's scripts/dataset_mean.py:50-70 on whole frames: ToTensor's fp32 x / 255, batches summed in fp32
    along the batch axis, fp32 squares, float64 accumulators per pixel, then the mean over pixels -> (mean, var) float64 [3]"""
    x = u8.numpy()
    n, h, w, _ = x.shape
    acc = np.zeros((3, h, w))
    sq_acc = np.zeros((3, h, w))
    for i in range(0, n, batch):
        imgs = np.transpose(x[i:i + batch], (0, 3, 1, 2)).astype(np.float32) / np.float32(255)  # ToTensor: fp32 division
        acc += np.sum(imgs, axis=0, dtype=np.float32)
        sq_acc += np.sum(imgs ** 2, axis=0, dtype=np.float32)
    N = n * h * w
    mean_p = np.asarray([np.sum(acc[c]) for c in range(3)]) / N
    std_p = np.asarray([np.sum(sq_acc[c]) for c in range(3)]) / N - mean_p ** 2
    return mean_p, std_p


MEAN_BOUND, VAR_BOUND = 8 * 2.0 ** -24, 26 * 2.0 ** -24  # fp32 roundings of the reference at 2^-24 each (see check_against_reference)


def check_against_reference(lib, dev):
    """|mean - reference| <= 8 * 2^-24: one fp32 division and at most seven fp32 adds per batch of 8, values in [0, 1];
    |var - reference| <= 26 * 2^-24: three roundings per square and seven adds on E[x^2] (10), twice the mean's error on mean^2 (16)"""
    from geomapnet_amd import pixel_sums
    cases = {"random": frames(20, 12, 17, seed=220), "dark": frames(20, 12, 17, seed=221, lo=0, hi=8),
             "bright": frames(20, 12, 17, seed=222, lo=200, hi=256), "saturated": torch.full((20, 12, 17, 3), 255, dtype=torch.uint8)}
    for name, u8 in cases.items():
        s = pixel_sums(u8.to(dev), _binding=lib)
        rm, rv = reference_stats(u8)
        dm, dv = np.abs(s.mean() - rm).max(), np.abs(s.var() - rv).max()
        print("%s: |mean - reference| %.3g (bound %.3g), |var - reference| %.3g (bound %.3g)" % (name, dm, MEAN_BOUND, dv, VAR_BOUND))
        assert dm <= MEAN_BOUND, (name, dm)
        assert dv <= VAR_BOUND, (name, dv)
