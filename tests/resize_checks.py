"""Backend-agnostic checks of the device Resize (csrc/resize.h, mn_set_input_resize, mn_op_resize_u8): each takes a Binding (`lib`)
and a torch device, so the CPU suite runs them on the SIMT-emulator build and the GPU suite on libmapnet_hip.so.  The reference is
tests/resize_ref.py (pinned to Pillow by test_device_resize.py).  Every comparison is bit for bit: pixels against resize_ref, and a
pass, step or gradient with the resize on against the same call on frames resized beforehand by resize_ref."""
import ctypes as C
import os

import numpy as np
import torch

import checks
import resize_ref
from geomapnet_amd._binding import MapNetHipError, ptr
from geomapnet_amd.data import resize_dims

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def frames(n, h, w, seed, binary=False):
    """uint8 [n, h, w, 3]: uniform noise, or only 0 and 255"""
    gen = torch.Generator().manual_seed(seed)
    if binary:
        return torch.randint(0, 2, (n, h, w, 3), generator=gen, dtype=torch.uint8) * 255
    return torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.uint8)


_REF = {}


def ref(u8, H, W):
    """resize_ref.resize as a uint8 tensor, computed once per (frames, size) and shared; callers leave it unchanged"""
    key = (u8.data_ptr(), tuple(u8.shape), H, W)
    if key not in _REF:
        _REF[key] = (u8, torch.from_numpy(resize_ref.resize(u8.numpy(), H, W)))
    return _REF[key][1]


def tile(lib, sh, sw, H, W):
    th, tw = C.c_int(), C.c_int()
    lib.check(lib.op_resize_tile(sh, sw, H, W, C.byref(th), C.byref(tw)))
    return th.value, tw.value


def run_op(lib, dev, u8, H, W):
    """mn_op_resize_u8 -> uint8 [B, H, W, 3]; the bytes around the output and the input are checked to be untouched"""
    B, sh, sw, _ = u8.shape
    x = u8.contiguous().to(dev)
    guard = 64
    buf = torch.full((B * H * W * 3 + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + B * H * W * 3]
    nwork = int(lib.op_resize_work_bytes(sh, sw, H, W))
    assert nwork > 0
    work = torch.zeros(nwork, dtype=torch.uint8, device=dev)
    lib.check(lib.op_resize_u8(ptr(x), ptr(out), ptr(work), B, sh, sw, H, W, None))
    checks.dev_sync(dev)
    b = buf.cpu()
    assert (b[:guard] == 0xA5).all() and (b[-guard:] == 0xA5).all(), "the kernel wrote outside its output"
    assert torch.equal(x.cpu(), u8), "the kernel wrote to its input"
    return b[guard:-guard].view(B, H, W, 3)


def check_op(lib, dev, B, sh, sw, H, W, seed=1, binary=False):
    u8 = frames(B, sh, sw, seed, binary)
    got = run_op(lib, dev, u8, H, W)
    want = ref(u8, H, W)
    bad = (got != want).nonzero()
    assert len(bad) == 0, ("%dx%d -> %dx%d: %d bytes differ, first at %s" % (sh, sw, H, W, len(bad), bad[0].tolist()))


RAGGED = ((37, 53, 16, 22), (53, 37, 22, 16), (20, 31, 32, 49), (61, 97, 16, 25), (48, 64, 48, 40), (48, 64, 30, 64))
# spans 3 x 3 tiles: at 75x300 -> 40x160 the host picks tiles of 16 output rows x 64 output columns (checked in the test)
MULTI_TILE = (75, 300, 40, 160)


def check_op_shapes(lib, dev, shapes=RAGGED, B=3):
    for k, (sh, sw, H, W) in enumerate(shapes):
        check_op(lib, dev, B, sh, sw, H, W, seed=20 + k)
        check_op(lib, dev, B, sh, sw, H, W, seed=40 + k, binary=True)


def check_multi_tile(lib, dev, B=3):
    sh, sw, H, W = MULTI_TILE
    th, tw = tile(lib, sh, sw, H, W)
    assert (th, tw) == (16, 64), (th, tw)
    assert -(-H // th) >= 3 and -(-W // tw) >= 3
    check_op(lib, dev, B, sh, sw, H, W, seed=60)
    check_op(lib, dev, B, sh, sw, H, W, seed=61, binary=True)


# ---- plan level -----------------------------------------------------------------------------------------------------------------
def model(lib, dev, dtype_name="fp32", mapnet=False, seed=7):
    import jitter_checks
    return jitter_checks.model(lib, dev, dtype_name, mapnet, seed)


def engine(net):
    return (net.mapnet if hasattr(net, "mapnet") else net)._engine


def forward(net, u8, training=False):
    net.train(training)
    with torch.no_grad():
        return net(u8.to(engine(net).device)).cpu()


def pair(lib, dev, dtype_name, size, mapnet=False):
    """two models of the same weights on uint8 input: `a` resizes on the device, `b` takes frames resized beforehand"""
    a, b = model(lib, dev, dtype_name, mapnet), model(lib, dev, dtype_name, mapnet)
    a.set_input_resize(size)
    return a, b


def check_forward(lib, dev, dtype_name="fp32", B=3, src=(48, 64), size=32, jitter=False):
    """forward with training 0 and 1 (and ColorJitter on: same seed and pass count, so the same draws): poses, the frames in the
    buffer and the draws equal those of the pre-resized call"""
    H, W = resize_dims(src[0], src[1], size)
    u8 = frames(B, src[0], src[1], seed=3)
    pre = ref(u8, H, W)
    a, b = pair(lib, dev, dtype_name, size)
    if jitter:
        for net in (a, b):
            net.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=11)
    for training in (False, True, False):
        pa, pb = forward(a, u8, training), forward(b, pre, training)
        assert torch.isfinite(pa).all()
        assert torch.equal(pa, pb), (training, (pa - pb).abs().max().item())
        ea, eb = engine(a), engine(b)
        plan_a = [p for p in ea.plans.values() if p["images"] == B][0]
        assert plan_a["src"] == tuple(src) and (plan_a["cfg"].H, plan_a["cfg"].W) == (H, W)
        assert torch.equal(ea.resized_frames(plan_a).cpu(), pre)
        if jitter:
            plan_b = [p for p in eb.plans.values() if p["images"] == B][0]
            assert torch.equal(ea.color_jitter_draws(plan_a), eb.color_jitter_draws(plan_b))
            assert ea.jitter_calls == eb.jitter_calls


def _train_setup(lib, dev, dtype_name, size, jitter):
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    _, net = checks.build_pair(lib, dev)
    net.set_input_u8(MEAN, STD)
    if size is not None:
        net.set_input_resize(size)
    if jitter:
        net.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=5)
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    net.train()
    return G, net, c, opt


def check_train_step(lib, dev, dtype_name="fp32", N=1, T=2, src=(48, 64), size=32, jitter=False):
    """one MapNet training step under MN_DETERMINISTIC=1: loss, poses, every parameter, the criterion's and BatchNorm's buffers after
    the step equal those of the step on pre-resized frames"""
    import oracle
    checks._fresh()
    H, W = resize_dims(src[0], src[1], size)
    u8 = frames(N * T, src[0], src[1], seed=4).view(N, T, src[0], src[1], 3)
    pre = ref(u8.view(-1, src[0], src[1], 3), H, W).view(N, T, H, W, 3)
    _, t = oracle.make_batch("mapnet", N, 8, 8, seed=7)
    t = t[:, :T] if t.shape[1] != T else t
    old = os.environ.get("MN_DETERMINISTIC")
    os.environ["MN_DETERMINISTIC"] = "1"
    try:
        res = []
        for x, sz in ((u8, size), (pre, None)):
            G, net, c, opt = _train_setup(lib, dev, dtype_name, sz, jitter)
            loss, poses = G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True)
            checks.dev_sync(dev)
            eng = engine(net)
            res.append((float(loss), poses.cpu().clone(), eng.params.cpu().clone(), eng.buffers.cpu().clone(), eng.jitter_calls))
    finally:
        os.environ.pop("MN_DETERMINISTIC", None)
        if old is not None:
            os.environ["MN_DETERMINISTIC"] = old
    (la, pa, wa, ba, ja), (lb, pb, wb, bb, jb) = res
    assert np.isfinite(la) and la == lb, (la, lb)
    assert torch.equal(pa, pb)
    assert torch.equal(wa, wb), (wa - wb).abs().max().item()
    assert torch.equal(ba, bb)
    assert ja == jb == (1 if jitter else 0)


def check_input_grad(lib, dev, dtype_name="fp32", B=2, src=(48, 64), size=32):
    """input_gradient and saliency stay at the network's H x W and equal those of the pre-resized call"""
    H, W = resize_dims(src[0], src[1], size)
    u8 = frames(B, src[0], src[1], seed=5)
    pre = ref(u8, H, W)
    a, b = pair(lib, dev, dtype_name, size)
    a.eval()
    b.eval()
    dev_ = engine(a).device
    ga, gb = a.input_gradient(u8.to(dev_)).cpu(), b.input_gradient(pre.to(dev_)).cpu()
    assert tuple(ga.shape) == (B, 3, H, W)
    assert torch.isfinite(ga).all() and ga.abs().max() > 0
    assert torch.equal(ga, gb)
    (pa, ma), (pb, mb) = a.saliency(u8.to(dev_)), b.saliency(pre.to(dev_))
    assert tuple(ma.shape) == (B, H, W)
    assert torch.equal(pa.cpu(), pb.cpu()) and torch.equal(ma.cpu(), mb.cpu())
    assert ma.max().item() == 1.0


def check_off_is_off(lib, dev, dtype_name="fp32", B=2, H=32, W=42):
    """set then unset -- through the model and on the plan itself -- equals the never-set model; another source size makes a second
    plan, and both plans stay valid"""
    u8 = frames(B, H, W, seed=6)
    never = model(lib, dev, dtype_name)
    want = forward(never, u8)
    a = model(lib, dev, dtype_name)
    a.set_input_resize(32)
    a.set_input_resize(None)
    assert torch.equal(forward(a, u8), want)
    assert all("src" not in p for p in engine(a).plans.values())
    # on the handle: on, a pass, off, a pass
    eng = engine(never)
    p = next(iter(eng.plans.values()))
    big = frames(B, 48, 64, seed=7)
    want_big = forward(never, ref(big, H, W))
    n = int(lib.input_resize_bytes(C.byref(p["cfg"]), 48, 64))
    assert n >= B * H * W * 3
    work = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    lib.check(lib.set_input_resize(p["handle"], 48, 64, ptr(work), n))
    big_dev, out = big.to(eng.device), torch.zeros(B, 6, dtype=torch.float32, device=eng.device)
    lib.check(lib.forward(p["handle"], ptr(big_dev), ptr(out), 0, None))
    checks.dev_sync(dev)
    assert torch.equal(out.cpu(), want_big)
    lib.check(lib.set_input_resize(p["handle"], 0, 0, None, 0))
    assert torch.equal(forward(never, u8), want)
    # two source sizes, one network size: two plans, used alternately
    b = model(lib, dev, dtype_name)
    b.set_input_resize((H, W))
    x1, x2 = frames(B, 48, 64, seed=8), frames(B, 40, 50, seed=9)
    pre = model(lib, dev, dtype_name)
    w1, w2 = forward(pre, ref(x1, H, W)), forward(pre, ref(x2, H, W))
    for _ in range(2):
        assert torch.equal(forward(b, x1), w1)
        assert torch.equal(forward(b, x2), w2)
    assert sorted(p["src"] for p in engine(b).plans.values()) == [(40, 50), (48, 64)]


def check_errors(lib, dev, H=32, W=42):
    """every refusal comes back as a message, before any launch"""
    # set_input_resize without set_input_u8
    net = model(lib, dev)
    net.set_input_u8(None)
    try:
        net.set_input_resize(32)
        raise AssertionError("set_input_resize without set_input_u8 must fail")
    except MapNetHipError as e:
        assert "set_input_u8" in str(e), str(e)
    for bad in (0, -3, (32, 0)):
        m = model(lib, dev)
        try:
            m.set_input_resize(bad)
            raise AssertionError("accepted size %r" % (bad,))
        except MapNetHipError:
            pass
    # a plan on fp32 input with the resize on: the forward pass fails, naming the cause
    x = torch.randn(2, 3, H, W)
    y = forward(net, x)
    eng = engine(net)
    p = next(iter(eng.plans.values()))
    h, cfg = p["handle"], p["cfg"]
    n = int(lib.input_resize_bytes(C.byref(cfg), 48, 64))
    work = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    lib.check(lib.set_input_resize(h, 48, 64, ptr(work), n))
    try:
        forward(net, x)
        raise AssertionError("fp32 input with the resize on must fail")
    except MapNetHipError as e:
        assert "uint8" in str(e) and "Resize" in str(e), str(e)
    lib.check(lib.set_input_resize(h, 0, 0, None, 0))
    assert torch.equal(forward(net, x), y)
    # the work buffer one byte short, missing, and bad sizes
    assert lib.set_input_resize(h, 48, 64, ptr(work), n - 1) != 0
    assert "mn_input_resize_bytes" in lib.last_error().decode()
    assert lib.set_input_resize(h, 48, 64, None, n) != 0
    assert "work" in lib.last_error().decode()
    for sh, sw in ((0, 64), (48, 0), (-1, 64), (48, -5)):
        assert lib.set_input_resize(h, sh, sw, ptr(work), n) != 0
        assert "positive" in lib.last_error().decode()
        assert lib.input_resize_bytes(C.byref(cfg), sh, sw) == -1
    assert lib.input_resize_bytes(C.byref(cfg), 0, 0) == -1
    assert torch.equal(forward(net, x), y)  # the refused calls changed nothing
    # the operator
    u8 = frames(1, 8, 8, seed=1).to(eng.device)
    out = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=eng.device)
    assert lib.op_resize_work_bytes(0, 8, 4, 4) == -1 and lib.op_resize_work_bytes(8, 8, 4, -1) == -1
    for args in ((0, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, -2)):
        assert lib.op_resize_u8(ptr(u8), ptr(out), ptr(work), *args, None) != 0
        assert "mn_op_resize_u8" in lib.last_error().decode()
    assert lib.op_resize_u8(ptr(u8), ptr(out), None, 1, 8, 8, 4, 4, None) != 0
    assert lib.op_resize_u8(None, ptr(out), ptr(work), 1, 8, 8, 4, 4, None) != 0
    checks.dev_sync(dev)
    assert not out.cpu().any()  # nothing was launched
