"""Backend-agnostic checks of the device ColorJitter (csrc/jitter.h, mn_set_color_jitter): each takes a Binding (`lib`) and a torch
device, so the CPU suite runs them on the SIMT-emulator build and the GPU suite on libmapnet_hip.so.  The reference is
tests/jitter_ref.py, a float64 restatement of torchvision's ColorJitter, fed the factors and order the device reports."""
import ctypes as C

import numpy as np
import torch

import checks
import jitter_ref
import oracle
from geomapnet_amd._binding import MapNetHipError, ptr

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
XPAD_TOL = 1e-5 / min(STD)  # fp32 arithmetic on [0, 1] values, then Normalize
ALL = (True, True, True, True)


def u8_frames(n, H, W, seed):
    return torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def run_op(lib, dev, u8, ranges, seed, call):
    """mn_op_color_jitter: -> (normalised jittered image [B, H, W, 3] float64, draws [B, 8] float64)"""
    B, H, W, _ = u8.shape
    x = u8.contiguous().to(dev)
    out = torch.zeros(B, H + 6, W + 6, 4, dtype=torch.float32, device=dev)
    draws = torch.zeros(B, 8, dtype=torch.float32, device=dev)
    work = torch.zeros(B * 9, dtype=torch.float32, device=dev)
    r, m, s = (C.c_float * 4)(*ranges), (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    lib.check(lib.op_color_jitter(ptr(x), ptr(out), ptr(draws), ptr(work), B, H, W, r, C.c_uint64(seed), C.c_uint32(call), m, s,
                                  None))
    checks.dev_sync(dev)
    out = out.cpu().double().numpy()
    assert not out[:, :3].any() and not out[:, -3:].any() and not out[:, :, :3].any() and not out[:, :, -3:].any()
    assert not out[..., 3].any()
    return out[:, 3:3 + H, 3:3 + W, :3], draws.cpu().double().numpy()


def model(lib, dev, dtype_name="fp32", mapnet=False, seed=7):
    """a PoseNet (or MapNet) on uint8 input, random weights"""
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    torch.manual_seed(seed)
    net = G.PoseNet(G.resnet34(_binding=lib), droprate=0.0, pretrained=False, _binding=lib)
    if mapnet:
        net = G.MapNet(net)
    if torch.device(dev).type == "cuda":
        net.cuda()
    net.set_input_u8(MEAN, STD)
    return net


def engine(net):
    return (net.mapnet if hasattr(net, "mapnet") else net)._engine


def last_plan(net, images):
    ps = [p for p in engine(net).plans.values() if p["images"] == images]
    assert len(ps) == 1
    return ps[0]


def xpad(net, plan, H, W):
    """the plan's normalised input [B, H, W, 3] as float64 (the padding checked to be zero)"""
    checks.dev_sync(engine(net).device)
    t = engine(net).debug_tensor(plan, "xpad").float().cpu().double().numpy()
    Hp, Wp = H + 6, (W + 8) & ~1
    t = t.reshape(plan["images"], Hp, Wp, 4)
    assert not t[:, :3].any() and not t[:, 3 + H:].any() and not t[:, :, :3].any() and not t[:, :, 3 + W:].any()
    assert not t[..., 3].any()
    return t[:, 3:3 + H, 3:3 + W, :3]


def forward(net, u8, training=False):
    net.train(training)
    with torch.no_grad():
        return net(u8.to(engine(net).device)).cpu()


def assert_matches(got, u8, draws, active=ALL, tol=XPAD_TOL, rel=0.0):
    ref = jitter_ref.jitter_u8_normalised(u8.numpy(), draws, MEAN, STD, active)
    err = np.abs(got - ref) - rel * np.abs(ref)
    assert err.max() <= tol, (err.max(), np.unravel_index(err.argmax(), err.shape), draws[np.unravel_index(err.argmax(), err.shape)[0]])


def check_single_ops(lib, dev, dtype_name="fp32", B=6, H=40, W=53, ranges=(0.7, 0.7, 0.7, 0.5), tol=XPAD_TOL, rel=0.0):
    """each op alone (the other ranges 0): xpad = the restatement given the reported factor; a skipped op reports identity"""
    u8 = u8_frames(B, H, W, seed=11)
    for op in range(4):
        net = model(lib, dev, dtype_name)
        r = [0.0] * 4
        r[op] = ranges[op]
        net.set_color_jitter(*r, seed=100 + op)
        forward(net, u8)
        p = last_plan(net, B)
        d = engine(net).color_jitter_draws(p).double().numpy()
        ident = np.array([1.0, 1.0, 1.0, 0.0])
        others = [k for k in range(4) if k != op]
        assert (d[:, others] == ident[others]).all(), d
        assert (d[:, op] != ident[op]).all(), d
        active = tuple(k == op for k in range(4))
        assert_matches(xpad(net, p, H, W), u8, d, active, tol, rel)


def check_all_ops(lib, dev, dtype_name="fp32", B=6, H=40, W=53, max_passes=40, tol=XPAD_TOL, rel=0.0, all_orders=True):
    """all four ops: passes until every one of the 24 orders has occurred (all_orders); every image of every pass matches"""
    u8 = u8_frames(B, H, W, seed=12)
    net = model(lib, dev, dtype_name)
    net.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=2024)
    seen = set()
    for k in range(max_passes):
        forward(net, u8, training=bool(k % 2))
        p = last_plan(net, B)
        d = engine(net).color_jitter_draws(p).double().numpy()
        assert_matches(xpad(net, p, H, W), u8, d, ALL, tol, rel)
        seen |= {tuple(int(v) for v in row[4:]) for row in d}
        if not all_orders or len(seen) == 24:
            return k + 1
    raise AssertionError("only %d of the 24 orders in %d passes" % (len(seen), max_passes))


def check_off_is_off(lib, dev, dtype_name="fp32", B=6, H=40, W=53):
    """jitter enabled then disabled, or enabled with every range 0: xpad and poses bitwise those of a model that never enabled it"""
    u8 = u8_frames(B, H, W, seed=13)
    ref_net = model(lib, dev, dtype_name)
    ref_poses = forward(ref_net, u8)
    ref_x = xpad(ref_net, last_plan(ref_net, B), H, W)
    a = model(lib, dev, dtype_name)
    a.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=1)
    jittered = forward(a, u8)
    assert not torch.equal(jittered, ref_poses)
    a.set_color_jitter()
    b = model(lib, dev, dtype_name)
    b.set_color_jitter(0.0, 0.0, 0.0, 0.0, seed=1)
    for net in (a, b):
        got = forward(net, u8)
        assert torch.equal(got, ref_poses)
        assert np.array_equal(xpad(net, last_plan(net, B), H, W), ref_x)


def check_draws(lib, dev, images=4096, ranges=(1.0, 0.7, 0.3, 0.5), seed=77):
    """the draws of `images` images: ranges (brightness 1 gives [0, 2]), mean and variance within 5 sigma of uniform, a chi-square
    over the 24 orders, hue symmetric; the same (seed, pass) gives the same bits, the next pass other draws"""
    u8 = u8_frames(images, 1, 1, seed=1)
    _, d = run_op(lib, dev, u8, ranges, seed, 0)
    n = images
    for k in range(4):
        lo, hi = (-ranges[3], ranges[3]) if k == 3 else (max(0.0, 1.0 - ranges[k]), 1.0 + ranges[k])
        v = d[:, k]
        assert v.min() >= lo and v.max() <= hi, (k, v.min(), v.max())
        w = hi - lo
        mu, var = (lo + hi) / 2, w * w / 12
        assert abs(v.mean() - mu) <= 5 * np.sqrt(var / n), (k, v.mean(), mu)
        # variance of the sample variance of U(0, w): (w^4 / 80 - w^4 / 144) / n
        assert abs(v.var() - var) <= 5 * np.sqrt((w ** 4 / 80 - w ** 4 / 144) / n), (k, v.var(), var)
    assert d[:, 0].min() < 0.01 and d[:, 0].max() > 1.99  # brightness 1: [0, 2]
    orders = {}
    for row in d[:, 4:].astype(np.int64):
        assert sorted(row) == [0, 1, 2, 3], row
        orders[tuple(row)] = orders.get(tuple(row), 0) + 1
    assert len(orders) == 24
    e = n / 24
    chi2 = sum((c - e) ** 2 / e for c in orders.values())
    assert chi2 < 49.7, chi2  # 23 degrees of freedom, p = 0.001
    h = d[:, 3]
    assert abs((h > 0).mean() - 0.5) <= 5 * np.sqrt(0.25 / n)
    pos, neg = h[h > 0], -h[h < 0]  # |h| distributed alike on both sides: U(0, hue), sd hue / sqrt(12)
    assert abs(pos.mean() - neg.mean()) <= 5 * ranges[3] / np.sqrt(12) * np.sqrt(1 / len(pos) + 1 / len(neg))
    _, d2 = run_op(lib, dev, u8, ranges, seed, 0)
    assert np.array_equal(d, d2)
    _, d3 = run_op(lib, dev, u8, ranges, seed, 1)
    assert not np.any(np.all(d3 == d, axis=1))
    _, d4 = run_op(lib, dev, u8, ranges, seed + 1, 0)
    assert not np.any(np.all(d4 == d, axis=1))
    # a draw depends on (seed, pass, image) alone: the first images of a smaller launch draw the same
    _, d5 = run_op(lib, dev, u8[:300], ranges, seed, 0)
    assert np.array_equal(d5, d[:300])


def check_op_orders(lib, dev, B=96, H=12, W=16, max_calls=8):
    """the jittered conversion on its own (mn_op_color_jitter), every image against the restatement, until all 24 orders have
    occurred -- contrast after hue and saturation included"""
    u8 = u8_frames(B, H, W, seed=14)
    seen = set()
    for call in range(max_calls):
        got, d = run_op(lib, dev, u8, (0.7, 0.7, 0.7, 0.5), 9, call)
        assert_matches(got, u8, d)
        seen |= {tuple(int(v) for v in row[4:]) for row in d}
        if len(seen) == 24:
            return
    raise AssertionError("only %d orders" % len(seen))


def check_sequence(lib, dev, B=6, H=40, W=53):
    """the pass count: two passes of one plan draw (seed, 0) and (seed, 1); a second plan (a last batch of 2) continues with pass
    2; set_color_jitter_calls(0) replays pass 0 bit for bit"""
    u8 = u8_frames(B, H, W, seed=15)
    ranges, seed = (0.7, 0.7, 0.7, 0.5), 31
    net = model(lib, dev)
    net.set_color_jitter(*ranges, seed=seed)
    eng = engine(net)
    forward(net, u8)
    p = last_plan(net, B)
    d0 = eng.color_jitter_draws(p).double().numpy()
    x0 = xpad(net, p, H, W)
    exp, dexp = run_op(lib, dev, u8, ranges, seed, 0)
    assert np.array_equal(d0, dexp)
    assert np.abs(x0 - exp).max() <= XPAD_TOL
    forward(net, u8, training=True)
    d1 = eng.color_jitter_draws(p).double().numpy()
    assert np.array_equal(d1, run_op(lib, dev, u8, ranges, seed, 1)[1])
    assert not np.any(np.all(d1 == d0, axis=1))
    forward(net, u8[:2])
    q = last_plan(net, 2)
    assert np.array_equal(eng.color_jitter_draws(q).double().numpy(), run_op(lib, dev, u8, ranges, seed, 2)[1][:2])
    assert eng.jitter_calls == 3
    eng.set_color_jitter_calls(0)
    forward(net, u8)
    assert np.array_equal(eng.color_jitter_draws(p).double().numpy(), d0)
    assert np.array_equal(xpad(net, p, H, W), x0)


def check_errors(lib, dev, H=32, W=32):
    """jitter with fp32 input fails through the library, naming the cause; out-of-range settings are rejected"""
    net = model(lib, dev)
    net.set_input_u8(None)
    net.set_color_jitter(0.5, 0.0, 0.0, 0.0, seed=1)
    x = torch.randn(2, 3, H, W, device=engine(net).device)
    try:
        forward(net, x)
        raise AssertionError("fp32 input with ColorJitter must fail")
    except MapNetHipError as e:
        assert "uint8" in str(e), str(e)
    for bad in ((0.0, 0.0, 0.0, 0.6), (-0.1, 0.0, 0.0, 0.0), (float("nan"), 0.0, 0.0, 0.0), (0.0, float("inf"), 0.0, 0.0)):
        try:
            net.set_color_jitter(*bad)
            raise AssertionError("accepted %r" % (bad,))
        except MapNetHipError:
            pass
        h = next(iter(engine(net).plans.values()))["handle"]
        assert lib.set_color_jitter(h, *[C.c_float(v) for v in bad], C.c_uint64(0)) != 0
        assert "mn_set_color_jitter" in lib.last_error().decode()


def check_train_step(lib, dev, dtype_name="fp32", N=2, T=3, H=64, W=85, loss_rtol=1e-4, pose_atol=1e-3):
    """one MapNet training step with jitter on vs the oracle on the frames jittered host-side (jitter_ref) with the device's draws"""
    checks._fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    onet, net = checks.build_pair(lib, dev)
    u8 = u8_frames(N * T, H, W, seed=16).view(N, T, H, W, 3)
    _, t = oracle.make_batch("mapnet", N, 8, 8, seed=7)
    net.set_input_u8(MEAN, STD)
    net.set_color_jitter(0.7, 0.7, 0.7, 0.5, seed=3)
    oc = oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True)
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    oopt = oracle.Optimizer([{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}], "adam",
                            base_lr=1e-4, weight_decay=5e-4)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    onet.train()
    net.train()
    l, p = G.step_feedfwd(u8.to(dev), net, dev != "cpu", t.to(dev), c, opt, True)
    eng = engine(net)
    d = eng.color_jitter_draws(last_plan(net, N * T)).double().numpy()
    assert len({tuple(r) for r in d[:, :4].tolist()}) == N * T  # every frame its own draw
    x = jitter_ref.jitter_u8_normalised(u8.view(-1, H, W, 3).numpy(), d, MEAN, STD)
    x = torch.from_numpy(x).float().permute(0, 3, 1, 2).contiguous().view(N, T, 3, H, W)
    lo, po = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True)
    assert abs(l - lo) <= loss_rtol * max(1.0, abs(lo)), (l, lo)
    err = (p.cpu() - po.detach()).abs().max().item()
    assert err <= pose_atol * max(1.0, po.abs().max().item()), err
    return l, lo, err
