"""Backend-agnostic checks of the inference input gradient (csrc/input_grad.h, mn_input_grad): each takes a Binding (`lib`) and a
torch device, so the CPU suite runs them on the SIMT-emulator build and the GPU suite on libmapnet_hip.so."""
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

import checks
import oracle
from checks import K, TD, OUT_TOL
from geomapnet_amd._binding import MapNetHipError

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- operators ---------------------------------------------------------------------------------------------------------------------
def run_stem_dgrad(lib, dev, dtype, gy_nchw, w_oihw, B, H, W, alpha=1.0):
    td = TD[dtype]
    gy = gy_nchw.permute(0, 2, 3, 1).contiguous().to(td).to(dev)
    w = w_oihw.permute(0, 2, 3, 1).contiguous().float().to(dev)  # OHWI fp32, the parameter arena's layout
    out = torch.full((B, 3, H, W), 7.0, dtype=torch.float32, device=dev)  # poison: every element must be written
    lib.check(lib.op_stem_dgrad(dtype, K(gy), K(w), K(out), B, H, W, checks.f32(alpha), None))
    checks.dev_sync(dev)
    return out.cpu().double()


def check_stem_dgrad(lib, dev, dtype, B, H, W, seed=31):
    """mn_op_stem_dgrad vs float64 torch.nn.grad.conv2d_input on the same (fp16: fp16-rounded) gy and weights, at the tolerance of
    checks.check_conv_dgrad_op for the dtype; then one-hot gy at the four corners: exact 7x7 footprints (a single product each)."""
    checks._fresh()
    gen = torch.Generator().manual_seed(seed)
    H0, W0 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = checks.q_op(torch.randn(B, 64, H0, W0, generator=gen), dtype)
    w = checks.q_op(torch.randn(64, 3, 7, 7, generator=gen) * 0.1, dtype)
    want = torch.nn.grad.conv2d_input((B, 3, H, W), w.double(), gy.double(), stride=2, padding=3)
    got = run_stem_dgrad(lib, dev, dtype, gy, w, B, H, W)
    err = (got - want).abs().max().item()
    print("stem_dgrad dtype %d (%d,%d,%d): max err %.3e, max |want| %.3e" % (dtype, B, H, W, err, want.abs().max().item()))
    assert err <= OUT_TOL[dtype] * want.abs().max().item() + 1e-6, err
    # alpha scales the result
    got2 = run_stem_dgrad(lib, dev, dtype, gy, w, B, H, W, alpha=0.25)
    assert torch.equal(got2, got * 0.25)
    # corners: one gy element each, weights exactly representable in fp16 -> every output is one exact product or zero
    wi = (torch.randint(-8, 9, (64, 3, 7, 7), generator=gen).float() / 8.0)
    for (p, q) in ((0, 0), (0, W0 - 1), (H0 - 1, 0), (H0 - 1, W0 - 1)):
        g1 = torch.zeros(B, 64, H0, W0)
        g1[B - 1, 5 + p % 3, p, q] = 2.0
        want1 = torch.nn.grad.conv2d_input((B, 3, H, W), wi.double(), g1.double(), stride=2, padding=3)
        got1 = run_stem_dgrad(lib, dev, dtype, g1, wi, B, H, W)
        assert torch.equal(got1, want1), (p, q)
        nz = got1[B - 1].abs().sum(0).nonzero()
        assert nz[:, 0].min() >= 2 * p - 3 and nz[:, 0].max() <= 2 * p + 3 and nz[:, 1].min() >= 2 * q - 3 and nz[:, 1].max() <= 2 * q + 3


def check_bn_eval_bwd(lib, dev, dtype, M=1031, Cc=64, seed=33):
    """gy = (gate > 0 ? g : 0) * scale[c]: bit-equal to the fp32 restatement for fp32, the fp32 product rounded once for fp16; with a
    gate and without; M = 1031 rows are no multiple of the 256-thread workgroup's pieces"""
    checks._fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(M, Cc, generator=gen).to(td)
    gate = torch.relu(torch.randn(M, Cc, generator=gen)).to(td)
    scale = (torch.rand(Cc, generator=gen) + 0.5) * torch.where(torch.rand(Cc, generator=gen) < 0.2, -1.0, 1.0)
    for use_gate in (True, False):
        out = torch.full((M, Cc), 7.0, dtype=td, device=dev)
        lib.check(lib.op_bn_eval_bwd(dtype, K(g.to(dev)), K(gate.to(dev)) if use_gate else None, K(scale.to(dev)), K(out), M, Cc, None))
        checks.dev_sync(dev)
        gg = torch.where(gate.float() > 0, g.float(), torch.zeros(())) if use_gate else g.float()
        want = (gg * scale[None, :]).to(td)
        assert torch.equal(out.cpu(), want), (dtype, use_gate, (out.cpu().float() - want.float()).abs().max().item())


def saliency_ref(gx, x):
    """numpy float32 restatement of plot_activations.py:130-133 per image (a constant map -> zeros)"""
    gx, x = gx.numpy().astype(np.float32), x.numpy().astype(np.float32)
    out = np.zeros((gx.shape[0],) + gx.shape[2:], dtype=np.float32)
    for b in range(gx.shape[0]):
        act = np.amax(np.abs(gx[b] * x[b]), axis=0)
        act = act - act.min()
        m = act.max()
        out[b] = act / m if m > 0 else np.zeros_like(act)
    return out


def check_saliency_op(lib, dev, B=3, H=33, W=47, seed=35):
    checks._fresh()
    gen = torch.Generator().manual_seed(seed)
    gx = torch.randn(B, 3, H, W, generator=gen) * torch.tensor([1e-3, 1.0, 50.0])[:B, None, None, None]  # another range per image
    x = torch.randn(B, 3, H, W, generator=gen)
    cases = [(gx, x), (torch.ones(1, 3, H, W), torch.full((1, 3, H, W), 0.5))]  # the second: a constant image -> all zeros
    for g, xx in cases:
        n = g.shape[0]
        out = torch.full((n, H, W), 7.0, dtype=torch.float32, device=dev)
        work = torch.zeros(int(lib.op_saliency_work_floats(n)), dtype=torch.float32, device=dev)
        lib.check(lib.op_saliency(K(g.to(dev)), K(xx.to(dev)), K(out), K(work), n, H, W, None))
        checks.dev_sync(dev)
        want = saliency_ref(g, xx)
        assert np.array_equal(out.cpu().numpy(), want)
    assert not want.any()


# ---- the whole call against the oracle -------------------------------------------------------------------------------------------------
def pair(lib, dev, dtype_name, seed=7):
    """oracle and library MapNet with the same weights and randomised running statistics, both in eval mode"""
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    onet, net = checks.build_pair(lib, dev, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    sd = onet.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(0.1 * torch.randn(v.shape, generator=gen))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=gen))
    net.load_state_dict(sd)
    onet.eval()
    net.eval()
    return onet, net


def rel_l2(a, b):
    """per-image relative L2 of a against b, [N, ...] -> list"""
    a, b = a.double().flatten(1), b.double().flatten(1)
    return ((a - b).norm(dim=1) / b.norm(dim=1)).tolist()


def oracle_grad(onet, x, cot=None):
    x = x.clone().requires_grad_()
    out = onet(x)
    if cot is None:
        out.mean().backward()
        return x.grad.detach(), out.detach()
    return torch.autograd.grad(out, x, cot.to(out.dtype))[0].detach(), out.detach()


class _Store16(torch.autograd.Function):
    """a tensor the fp16 plan keeps in fp16: value rounded forward, gradient rounded (under the loss scale) on the way back
    (tools/fp16_budget_backward.py)"""

    @staticmethod
    def forward(ctx, t, scale):
        ctx.scale = scale
        return t.half().float()

    @staticmethod
    def backward(ctx, g):
        return (g * ctx.scale).half().float() / ctx.scale, None


def oracle_fp16_storage(onet, x, scale, cot=None):
    """the oracle's own eval forward and backward pass with every stored conv / BatchNorm / ReLU output rounded to fp16 and its
    gradient rounded to fp16 under the loss scale; weights as fp16 operand copies"""
    st = lambda t: _Store16.apply(t, scale)  # noqa: E731
    w16 = lambda w: w.half().float()  # noqa: E731
    bn = lambda t, m: F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)  # noqa: E731
    pn = onet.mapnet
    fe = pn.feature_extractor
    n, t = x.shape[:2]
    xin = x.reshape(n * t, *x.shape[2:]).clone().requires_grad_()
    y = st(F.conv2d(xin.detach().half().float() + (xin - xin.detach()), w16(fe.conv1.weight), None, 2, 3))
    a = st(F.max_pool2d(st(F.relu(bn(y, fe.bn1))), 3, 2, 1))
    for li in range(1, 5):
        for blk in getattr(fe, "layer%d" % li):
            y1 = st(F.conv2d(a, w16(blk.conv1.weight), None, blk.conv1.stride, 1))
            a1 = st(F.relu(bn(y1, blk.bn1)))
            y2 = st(F.conv2d(a1, w16(blk.conv2.weight), None, 1, 1))
            z = bn(y2, blk.bn2)
            if blk.downsample is not None:
                sc = st(bn(st(F.conv2d(a, w16(blk.downsample[0].weight), None, blk.downsample[0].stride, 0)), blk.downsample[1]))
            else:
                sc = a
            a = st(F.relu(z + sc))
    feat = F.relu(F.linear(a.mean((2, 3)), fe.fc.weight, fe.fc.bias))
    out = torch.cat((F.linear(feat, pn.fc_xyz.weight, pn.fc_xyz.bias), F.linear(feat, pn.fc_wpqr.weight, pn.fc_wpqr.bias)), 1)
    if cot is None:
        out.mean().backward()
        g = xin.grad
    else:
        g = torch.autograd.grad(out, xin, cot.reshape(-1, 6))[0]
    return g.detach().view(x.shape)


def check_input_grad_vs_oracle(lib, dev, dtype_name, N=1, T=2, H=40, W=53, seed=7, cotangent=False):
    """MapNet.input_gradient vs the oracle's autograd in eval mode.  Metric: per-image relative L2 against the oracle evaluated in
    float64.  fp32: bound 4 x the same metric of the fp32 oracle (two independent fp32 evaluations may each sit that far from
    float64, x 2 for other summation orders).  fp16: bound 1.5 x the deviation of the oracle itself with fp16 storage
    (oracle_fp16_storage).  The poses the call returns are those of net(x) in eval mode, bit for bit."""
    checks._fresh()
    onet, net = pair(lib, dev, dtype_name, seed=seed)
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(N, T, 3, H, W, generator=gen)
    cot = torch.randn(N, T, 6, generator=gen) if cotangent else None
    o64 = copy.deepcopy(onet).double()
    g64, _ = oracle_grad(o64, x.double(), cot)
    g32, _ = oracle_grad(onet, x, cot)
    floor32 = rel_l2(g32.flatten(0, 1), g64.flatten(0, 1))
    got = net.input_gradient(x.to(dev), None if cot is None else cot.to(dev))
    assert got.shape == x.shape and got.dtype == torch.float32
    dev_err = rel_l2(got.cpu().flatten(0, 1), g64.flatten(0, 1))
    if dtype_name == "fp16":
        scale = net.mapnet._engine.loss_scale_state()[0]
        g16 = oracle_fp16_storage(onet, x, scale, cot)
        floor = rel_l2(g16.flatten(0, 1), g64.flatten(0, 1))
        bound = [1.5 * f for f in floor]
    else:
        floor = floor32
        bound = [4.0 * f for f in floor32]
    print("input_grad %s (%d,%d,%d,%d) cot=%s: device %s, floor %s" % (dtype_name, N, T, H, W, cotangent,
                                                                       ["%.3e" % v for v in dev_err], ["%.3e" % v for v in floor]))
    checks._record_deviation({"check": "input_grad", "dtype": dtype_name, "N": N, "T": T, "H": H, "W": W, "cot": bool(cotangent),
                              "device_rel_l2": dev_err, "floor_rel_l2": floor, "dev": str(dev)})
    for d, b in zip(dev_err, bound):
        assert d <= b, (dev_err, bound)
    # poses of the call = the eval forward pass, bit for bit; the maps are the restatement of the gradient the call produced
    poses, maps = net.saliency(x.to(dev))
    assert torch.equal(poses.cpu(), net(x.to(dev)).cpu())
    if cot is None:
        want = saliency_ref(got.cpu().flatten(0, 1), x.flatten(0, 1))
        assert np.array_equal(maps.cpu().flatten(0, 1).numpy(), want)


def check_u8_input(lib, dev, H=40, W=53, seed=7):
    """uint8 frames: the gradient with respect to the NORMALISED image = the fp32 path's gradient at that image, bit for bit (the
    same launches after the input conversion), and the maps use the image as the conversion computes it"""
    checks._fresh()
    _, net = pair(lib, dev, "fp32", seed=seed)
    net = net.mapnet
    u8 = torch.randint(0, 256, (1, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    scale = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float32)
    shift = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float32)
    xn = (u8.float() * scale + shift).permute(0, 3, 1, 2).contiguous()
    g_f = net.input_gradient(xn.to(dev)).cpu()
    net.set_input_u8(MEAN, STD)
    g_u = net.input_gradient(u8.to(dev)).cpu()
    _, maps = net.saliency(u8.to(dev))
    net.set_input_u8(None)
    # (the device conversion may contract its multiply-add: the images can differ in the last bit, the gradients by a few ulps)
    assert max(rel_l2(g_u, g_f)) <= 1e-5
    want = saliency_ref(g_u, xn)
    assert np.abs(maps.cpu().numpy() - want).max() <= 1e-5


def _state(net):
    eng = net.mapnet._engine
    checks.dev_sync(eng.device)
    st = {"params": eng.params.clone(), "opt": eng.opt_state.clone(), "buffers": eng.buffers.clone(), "step": eng.effective_step(),
          "jitter_calls": eng.jitter_calls, "scale": eng.loss_scale_state()}
    return st


def check_leaves_training_state(lib, dev, dtype_name="fp32", N=1, T=2, H=40, W=53):
    """(MN_DETERMINISTIC=1 set by the caller before the library read its knobs) train step, snapshot, input_gradient: parameters,
    gradient arena and moments, buffers, step count, pass counters and loss-scale state are bit-equal to the snapshot, and the next
    train step's loss and poses are bit-equal to those of a twin that never called input_gradient"""
    checks._fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)

    def make():
        onet, net = checks.build_pair(lib, dev)
        c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
        opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                          base_lr=1e-4, weight_decay=5e-4)
        net.train()
        return net, c, opt

    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    cuda = torch.device(dev).type == "cuda"
    runs = []
    for probe in (True, False):
        net, c, opt = make()
        G.step_feedfwd(x.to(dev), net, cuda, t.to(dev), c, opt, True, 0.0)
        if probe:
            before = _state(net)
            net.eval()
            g = net.input_gradient(x.to(dev))
            assert torch.isfinite(g).all() and g.abs().max() > 0
            net.train()
            after = _state(net)
            for k in before:
                same = torch.equal(before[k], after[k]) if torch.is_tensor(before[k]) else before[k] == after[k]
                assert same, k
        l, p = G.step_feedfwd(x.to(dev), net, cuda, t.to(dev), c, opt, True, 0.0)
        runs.append((float(l), p.cpu().clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def check_errors(lib, dev):
    checks._fresh()
    import geomapnet_amd as G
    _, net = pair(lib, dev, "fp32")
    x = torch.randn(1, 2, 3, 32, 40).to(dev)
    net.train()
    try:
        net.input_gradient(x)
        raise AssertionError("train mode must raise")
    except RuntimeError as e:
        assert "eval" in str(e)
    net.eval()
    try:
        net.input_gradient(x, torch.zeros(1, 2, 5))
        raise AssertionError("a cotangent of the wrong shape must raise")
    except ValueError as e:
        assert "cotangent" in str(e)
    pn = net.mapnet
    pn.set_input_u8(MEAN, STD)
    pn.set_color_jitter(0.4, 0.4, 0.4, 0.1, seed=3)
    u8 = torch.randint(0, 256, (1, 32, 40, 3), dtype=torch.uint8).to(dev)
    try:
        pn.input_gradient(u8)
        raise AssertionError("jitter on must raise")
    except MapNetHipError as e:
        assert "un-jittered" in str(e)
    # the library itself refuses as well (C callers)
    eng = pn._engine
    p = eng.plan(0, 1, 1, 32, 40)
    gx = torch.zeros(1, 3, 32, 40, device=dev)
    assert lib.input_grad(p["handle"], checks.ptr(u8), None, checks.ptr(gx), None, None, None) != 0
    assert "un-jittered" in lib.last_error().decode()
    pn.set_color_jitter()
    pn.set_input_u8(None)
    G.set_compute_dtype("fp16x2m")
    try:
        _, net2 = checks.build_pair(lib, dev)
        net2.eval()
        try:
            net2.input_gradient(x)
            raise AssertionError("fp16x2m must raise")
        except MapNetHipError as e:
            assert "fp32" in str(e) and "fp16" in str(e)
        eng2 = net2.mapnet._engine
        p2 = eng2.plan(0, 2, 1, 32, 40)
        gx2 = torch.zeros(2, 3, 32, 40, device=dev)
        assert lib.input_grad(p2["handle"], checks.ptr(x), None, checks.ptr(gx2), None, None, None) != 0
        assert "MN_DTYPE_F32" in lib.last_error().decode()
    finally:
        G.set_compute_dtype("fp32")
