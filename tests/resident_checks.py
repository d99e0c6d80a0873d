"""Backend-agnostic checks of the device-resident frame store (csrc/gather.h, the indexed resize_u8_kernel, mn_set_input_index,
geomapnet_amd/resident.py): each takes a Binding (`lib`) and a torch device, so the CPU suite runs them on the SIMT-emulator build
and the GPU suite on libmapnet_hip.so.  Gathering is a copy: every comparison is bit for bit against the tensor `store[index]`."""
import ctypes as C

import numpy as np
import torch

import checks
import resize_checks as RC
from geomapnet_amd._binding import MapNetHipError, ptr
from geomapnet_amd.resident import IndexedFrames

MEAN, STD = RC.MEAN, RC.STD
SENTINEL = 0xA5
GUARD = 64


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _flag(dev, value=7.0):
    """the bad-index flag, preset so that a call which does not clear it shows"""
    return torch.full((1,), value, dtype=torch.float32, device=dev)


# ---- mn_op_gather_frames ----------------------------------------------------------------------------------------------------------
def frame_bytes_of(case):
    """(frame_bytes, byte image [frames, frame_bytes] of `frames` random frames) for a case (h, w, fp32)"""
    h, w, fp32 = case
    return h * w * 3 * (4 if fp32 else 1)


def store_bytes(case, frames, seed):
    h, w, fp32 = case
    g = torch.Generator().manual_seed(seed)
    if fp32:
        return torch.randn(frames, 3, h, w, generator=g).view(torch.uint8).reshape(frames, -1).contiguous()
    return torch.randint(0, 256, (frames, h * w * 3), generator=g, dtype=torch.uint8)


# (h, w, fp32): 4653 odd; 6360 a multiple of 8, not of 16; 3840 a multiple of 16; 18612 fp32 frames
GATHER_CASES = ((33, 47, False), (40, 53, False), (32, 40, False), (33, 47, True))
GATHER_INDEX = (6, 4, 4, 1, 0)  # a repeated index, descending order
# index[b] == b: with store and output at the SAME offset mod 16 every frame then shares its alignment with its destination and takes
# the 16-byte pieces -- the path of every real frame size -- also where an odd frame size leaves a ragged head and tail
GATHER_INDEX_IN_PLACE = (0, 1, 2, 3, 4)


def run_gather(lib, dev, host, index, store_off=0, out_off=0, flag=None):
    """mn_op_gather_frames on a store / an output that start `store_off` / `out_off` bytes into their allocations -> the output
    bytes [images, frame_bytes]; the bytes around the output keep their sentinel and the store is unchanged"""
    frames, fb = host.shape
    n = len(index)
    sbuf = torch.zeros(store_off + frames * fb, dtype=torch.uint8, device=dev)
    store = sbuf[store_off:]
    store.copy_(host.reshape(-1))
    obuf = torch.full((out_off + n * fb + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    out = obuf[out_off + GUARD: out_off + GUARD + n * fb]
    assert store.data_ptr() % 16 == store_off % 16 and out.data_ptr() % 16 == (out_off + GUARD) % 16
    idx = _i32(list(index), dev)
    flag = _flag(dev) if flag is None else flag
    lib.check(lib.op_gather_frames(ptr(store), ptr(idx), ptr(out), fb, n, frames, ptr(flag), None))
    checks.dev_sync(dev)
    b = obuf.cpu()
    assert (b[:out_off + GUARD] == SENTINEL).all() and (b[out_off + GUARD + n * fb:] == SENTINEL).all(), \
        "the kernel wrote outside its output"
    assert torch.equal(store.cpu(), host.reshape(-1)), "the kernel wrote to the store"
    return b[out_off + GUARD: out_off + GUARD + n * fb].view(n, fb), flag.cpu().item()


def check_gather_case(lib, dev, case, seed=1):
    host = store_bytes(case, 7, seed)
    assert host.shape[1] == frame_bytes_of(case)
    want = host[list(GATHER_INDEX)]
    for store_off, out_off in ((1, 0), (5, 0), (0, 1), (0, 5)):
        got, flag = run_gather(lib, dev, host, GATHER_INDEX, store_off, out_off)
        bad = (got != want).nonzero()
        assert len(bad) == 0, ("frame_bytes %d, store +%d, out +%d: %d bytes differ, first at %s"
                               % (host.shape[1], store_off, out_off, len(bad), bad[0].tolist()))
        assert flag == 0.0, "a clean call must clear the flag"
    for store_off, out_off in ((0, 0), (19, 3)):  # (the output begins GUARD = 64 bytes behind out_off: both 0, or both 3, mod 16)
        for index in (GATHER_INDEX_IN_PLACE, GATHER_INDEX):
            got, flag = run_gather(lib, dev, host, index, store_off, out_off)
            assert torch.equal(got, host[list(index)]), (host.shape[1], store_off, out_off, index)
            assert flag == 0.0


# ---- mn_op_resize_u8_indexed ------------------------------------------------------------------------------------------------------
def run_resize_indexed(lib, dev, store, index, H, W, flag=None):
    """-> uint8 [images, H, W, 3]; the bytes around the output keep their sentinel"""
    F, sh, sw, _ = store.shape
    n = len(index)
    x = store.contiguous().to(dev)
    buf = torch.full((n * H * W * 3 + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    out = buf[GUARD:GUARD + n * H * W * 3]
    work = torch.zeros(int(lib.op_resize_work_bytes(sh, sw, H, W)), dtype=torch.uint8, device=dev)
    flag = _flag(dev) if flag is None else flag
    idx = _i32(list(index), dev)
    lib.check(lib.op_resize_u8_indexed(ptr(x), ptr(idx), F, ptr(out), ptr(work), n, sh, sw, H, W, ptr(flag), None))
    checks.dev_sync(dev)
    b = buf.cpu()
    assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), "the kernel wrote outside its output"
    return b[GUARD:-GUARD].view(n, H, W, 3), flag.cpu().item()


RESIZE_CASES = ((48, 64, 32, 43), (75, 100, 40, 53))
RESIZE_INDEX = (4, 0, 2)


def check_resize_indexed(lib, dev, sh, sw, H, W, seed=2):
    store = RC.frames(5, sh, sw, seed)
    got, flag = run_resize_indexed(lib, dev, store, RESIZE_INDEX, H, W)
    want = RC.run_op(lib, dev, store[list(RESIZE_INDEX)], H, W)  # the plain operator on host-gathered frames
    assert torch.equal(got, want), "%dx%d -> %dx%d: %d bytes differ" % (sh, sw, H, W, (got != want).sum().item())
    assert flag == 0.0


# ---- the bounds guard (emulator only: never aim a bad index at a shared GPU) -------------------------------------------------------
def check_bounds_guard(lib, dev):
    case = (33, 47, False)
    host = store_bytes(case, 7, seed=3)
    index = (-1, 2, 7, 5)
    got, flag = run_gather(lib, dev, host, index)
    assert flag == 1.0
    assert torch.equal(got, host[[0, 2, 0, 5]])
    _, flag = run_gather(lib, dev, host, (6, 0))
    assert flag == 0.0
    store = RC.frames(5, 48, 64, seed=4)
    got, flag = run_resize_indexed(lib, dev, store, (5, 3, -1), 32, 43)
    assert flag == 1.0
    assert torch.equal(got, RC.run_op(lib, dev, store[[0, 3, 0]], 32, 43))
    _, flag = run_resize_indexed(lib, dev, store, (4, 3), 32, 43)
    assert flag == 0.0


# ---- a store above 4 GiB (GPU only) -----------------------------------------------------------------------------------------------
def check_store_above_4gib(lib, dev):
    """470 000 frames of 48x64x3 bytes = 4.33 GB; only frame 0 and the last frame are written: the last frame's byte offset does
    not fit 32 bits"""
    F, sh, sw = 470000, 48, 64
    fb = sh * sw * 3
    assert (F - 1) * fb > 2 ** 32
    ends = RC.frames(2, sh, sw, seed=5)
    store = torch.empty(F, sh, sw, 3, dtype=torch.uint8, device=dev)
    store[0].copy_(ends[0])
    store[F - 1].copy_(ends[1])
    idx = _i32([F - 1, 0], dev)
    out = torch.full((2 * fb,), SENTINEL, dtype=torch.uint8, device=dev)
    flag = _flag(dev)
    lib.check(lib.op_gather_frames(ptr(store), ptr(idx), ptr(out), fb, 2, F, ptr(flag), None))
    checks.dev_sync(dev)
    assert torch.equal(out.cpu().view(2, sh, sw, 3), ends[[1, 0]])
    assert flag.item() == 0.0
    H, W = 32, 43
    work = torch.zeros(int(lib.op_resize_work_bytes(sh, sw, H, W)), dtype=torch.uint8, device=dev)
    res = torch.full((2 * H * W * 3,), SENTINEL, dtype=torch.uint8, device=dev)
    lib.check(lib.op_resize_u8_indexed(ptr(store), ptr(idx), F, ptr(res), ptr(work), 2, sh, sw, H, W, ptr(flag), None))
    checks.dev_sync(dev)
    del store
    assert torch.equal(res.cpu().view(2, H, W, 3), RC.run_op(lib, dev, ends[[1, 0]], H, W))
    assert flag.item() == 0.0


# ---- plan level: N = 1, T = 3, 40 x 53, a store of 6 frames -----------------------------------------------------------------------
PLAN_H, PLAN_W, PLAN_SRC, PLAN_INDEX = 40, 53, (75, 100), ((4, 1, 4),)

engine = RC.engine


def _net(lib, dev, dtype_name, u8=True):
    net = RC.model(lib, dev, dtype_name, mapnet=True)
    if not u8:
        net.set_input_u8(None)
    net.eval()
    return net


def _stores(dev):
    d = torch.device(dev)
    g = torch.Generator().manual_seed(11)
    return {"fp32": torch.randn(6, 3, PLAN_H, PLAN_W, generator=g).to(d),
            "u8": RC.frames(6, PLAN_H, PLAN_W, seed=12).to(d),
            "u8_src": RC.frames(6, PLAN_SRC[0], PLAN_SRC[1], seed=13).to(d)}


def _both(net, store, index=PLAN_INDEX):
    """-> (poses on IndexedFrames, poses on the tensor store[index]), on the host"""
    idx = torch.tensor(index, dtype=torch.int64)
    with torch.no_grad():
        a = net(IndexedFrames(store, idx)).cpu()
        b = net(store[idx.to(store.device)].contiguous()).cpu()
    return a, b


def check_plan_forward(lib, dev, dtype_name, form):
    """eval-mode poses of net(IndexedFrames(store, idx)) equal those of net(store[idx]) for one input form"""
    stores = _stores(dev)
    if form == "fp32":
        a, b = _both(_net(lib, dev, dtype_name, u8=False), stores["fp32"])
    elif form == "u8":
        a, b = _both(_net(lib, dev, dtype_name), stores["u8"])
    elif form == "u8_resize":
        net = _net(lib, dev, dtype_name)
        net.set_input_resize((PLAN_H, PLAN_W))
        a, b = _both(net, stores["u8_src"])
        assert all(p["src"] == PLAN_SRC for p in engine(net).plans.values())
        assert all("index_stage" not in p for p in engine(net).plans.values())  # the resample writes the batch: no staging
    elif form == "u8_jitter":
        res = []
        for indexed in (True, False):  # two models: the same seed and pass count, so the same draws
            net = _net(lib, dev, dtype_name)
            net.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=11)
            idx = torch.tensor(PLAN_INDEX, dtype=torch.int64)
            x = IndexedFrames(stores["u8"], idx) if indexed else stores["u8"][idx.to(stores["u8"].device)].contiguous()
            with torch.no_grad():
                poses = net(x).cpu()
            eng = engine(net)
            res.append((poses, eng.color_jitter_draws(next(iter(eng.plans.values()))), eng.jitter_calls))
        (a, da, ca), (b, db, cb) = res
        assert torch.equal(da, db) and ca == cb == 1
    else:
        raise ValueError(form)
    assert tuple(a.shape) == (1, 3, 6) and torch.isfinite(a).all()
    assert torch.equal(a, b), (form, (a - b).abs().max().item())


def check_plan_train_step(lib, dev, dtype_name):
    """after one step_feedfwd training step each way the network's padded input (`xpad`) is equal: the rest of the step is
    unchanged code"""
    import geomapnet_amd as G
    import oracle
    store = _stores(dev)["u8"]
    net = _net(lib, dev, dtype_name)
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    net.train()
    _, t = oracle.make_batch("mapnet", 1, 8, 8, seed=7)
    t = t[:, :3].to(dev)
    idx = torch.tensor(PLAN_INDEX, dtype=torch.int64)
    eng = engine(net)
    xpads = []
    for x in (store[idx.to(store.device)].contiguous(), IndexedFrames(store, idx)):
        loss, poses = G.step_feedfwd(x, net, dev != "cpu", t, c, opt, True)
        checks.dev_sync(dev)
        assert np.isfinite(loss) and tuple(poses.shape) == (1, 3, 6)
        plans = [p for p in eng.plans.values() if p["cfg"].mode == 1]
        assert len(plans) == 1
        xpads.append(eng.debug_tensor(plans[0], "xpad").clone().cpu())
    assert xpads[0].abs().max() > 0
    assert torch.equal(xpads[0], xpads[1])
    assert eng.input_index_bad(plans[0]) == 0.0


def check_plan_input_grad(lib, dev, dtype_name="fp32"):
    """input_gradient and saliency on IndexedFrames equal those on store[idx]"""
    store = _stores(dev)["u8"]
    net = _net(lib, dev, dtype_name)
    idx = torch.tensor(PLAN_INDEX, dtype=torch.int64)
    x, xi = store[idx.to(store.device)].contiguous(), IndexedFrames(store, idx)
    gb, pb, mb = engine(net).input_grad(x.view(3, PLAN_H, PLAN_W, 3), None, saliency=True)  # the tensor way: one pass gives all three
    ga = net.input_gradient(xi).cpu()
    assert tuple(ga.shape) == (1, 3, 3, PLAN_H, PLAN_W) and torch.isfinite(ga).all() and ga.abs().max() > 0
    assert torch.equal(ga.view(3, 3, PLAN_H, PLAN_W), gb.cpu())
    pa, ma = net.saliency(xi)
    assert tuple(ma.shape) == (1, 3, PLAN_H, PLAN_W) and ma.max().item() == 1.0
    assert torch.equal(pa.cpu().view(3, 6), pb.cpu()) and torch.equal(ma.cpu().view(3, PLAN_H, PLAN_W), mb.cpu())


def check_off_is_off(lib, dev, dtype_name="fp32", other_device="meta"):
    """an indexed pass leaves nothing behind in the plan; every refusal is a message (or a ValueError) before any launch"""
    store = _stores(dev)["u8"]
    net = _net(lib, dev, dtype_name)
    idx = torch.tensor(PLAN_INDEX, dtype=torch.int64)
    x = store[torch.tensor(((0, 2, 5),)).to(store.device)].contiguous()
    with torch.no_grad():
        before = net(x).cpu()
        eng = engine(net)
        p = next(iter(eng.plans.values()))
        nbytes = int(lib.plan_bytes(C.byref(p["cfg"])))
        net(IndexedFrames(store, idx))
        after = net(x).cpu()
    assert torch.equal(before, after)
    assert int(lib.plan_bytes(C.byref(p["cfg"]))) == nbytes and len(eng.plans) == 1
    assert eng.input_index_bad(p) == 0.0
    # the C entry: a NULL or short work, store_frames = 0, a misaligned index
    h, cfg = p["handle"], p["cfg"]
    need = int(lib.input_index_bytes(C.byref(cfg), 1))
    assert need == 3 * PLAN_H * PLAN_W * 3 and int(lib.input_index_bytes(C.byref(cfg), 0)) == 4 * need
    work = torch.zeros(need, dtype=torch.uint8, device=store.device)
    i32 = torch.zeros(4, dtype=torch.int32, device=store.device)
    for args, word in (((ptr(i32), 6, None, need), "work"), ((ptr(i32), 6, ptr(work), need - 1), "work"),
                       ((ptr(i32), 0, ptr(work), need), "store_frames"),
                       ((C.c_void_p(i32.data_ptr() + 2), 6, ptr(work), need), "index_dev")):
        assert lib.set_input_index(h, *args) != 0
        assert word in lib.last_error().decode(), (word, lib.last_error().decode())
    lib.check(lib.set_input_index(h, None, 0, None, 0))
    with torch.no_grad():
        assert torch.equal(net(x).cpu(), before)  # the refused calls changed nothing
    # an out-of-range host index
    for bad in (((0, 1, 6),), ((-1, 1, 2),)):
        try:
            IndexedFrames(store, torch.tensor(bad))
            raise AssertionError("accepted index %r" % (bad,))
        except ValueError as e:
            assert "6 frames" in str(e), str(e)
    # a store on another device
    elsewhere = torch.empty(6, PLAN_H, PLAN_W, 3, dtype=torch.uint8, device=other_device)
    try:
        net(IndexedFrames(elsewhere, idx))
        raise AssertionError("a store on another device must be refused")
    except RuntimeError as e:
        assert "model on" in str(e), str(e)
    # a store of another frame size than the plan
    small = RC.frames(6, PLAN_H - 8, PLAN_W, seed=14).to(store.device)
    try:
        eng.set_input_index(p, IndexedFrames(small, idx))
        raise AssertionError("a store of another frame size must be refused")
    except MapNetHipError as e:
        assert "frame" in str(e), str(e)
    with torch.no_grad():
        assert torch.equal(net(x).cpu(), before)
