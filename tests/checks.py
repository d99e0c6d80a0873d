"""Backend-agnostic parity checks.  Each takes a Binding (`lib`) and a torch device: the CPU suite
runs them on the SIMT-emulator build of the kernels (tests/test_emu_*.py), the GPU suite runs the
same checks on libmapnet_hip.so (tests/test_gpu_*.py, -m gpu).  References: torch CPU ops in fp64
(for single operators), the oracle (for the criteria / train step) and the committed golden vectors.
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

import oracle
from geomapnet_amd._binding import GatherGeom, ptr
from geomapnet_amd.posenet import _view

# dtype 2 = MN_DTYPE_F32X3: fp32 tensors, contraction on the f16 / bf16 matrix pipe with split (hi + lo) operands
# dtype 3 = MN_DTYPE_F16X2: conv operands / gates are h2 tensors (fp16 pairs, helpers below), everything else fp32
# dtype 4 = MN_DTYPE_F16X2M: the fp16 kernels (plain fp16 tensors) reading the HI halves of h2 gates / of an h2 weight-gradient X operand
TD = {0: torch.float32, 1: torch.float16, 2: torch.float32, 3: torch.float32, 4: torch.float16, 5: torch.float32}
# output rounding of the storage type relative to the largest output magnitude (x3: 2^-22 per product with fp16 halves,
# 2^-16 with the bf16 halves of the backward operators)
OUT_TOL = {0: 2e-5, 1: 2e-3, 2: 5e-5, 3: 2e-5}


def f32(x):
    return C.c_float(float(x))


_KEEP = []


def K(t):
    """pointer of a (possibly temporary) tensor, kept alive until the next check starts"""
    if t is None:
        return None
    _KEEP.append(t)
    return ptr(t)


_ZP = {}


def zero_page(dev):
    """256 zero bytes on `dev` (the conv kernels' source for out-of-image taps)"""
    key = str(dev)
    if key not in _ZP:
        _ZP[key] = torch.zeros(64, dtype=torch.float32, device=dev)
    return _ZP[key]


def _fresh():
    del _KEEP[:]


def dev_sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def fwd_geom(B, H, W, Cin, Cout, k, stride, pad):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = GatherGeom(B=B, Hi=H, Wi=W, C=Cin, P=Ho, Q=Wo, R=k, S=k, mul_p=stride, mul_q=stride, rsign=1, ssign=1,
                   off_h=-pad, off_w=-pad, div=1, M=B * Ho * Wo, N=Cout, K=k * k * Cin)
    return g, Ho, Wo


def dgrad_geom(B, H, W, Cin, Cout, k, stride, pad):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return GatherGeom(B=B, Hi=Ho, Wi=Wo, C=Cout, P=H, Q=W, R=k, S=k, mul_p=1, mul_q=1, rsign=-1, ssign=-1, off_h=pad,
                      off_w=pad, div=stride, M=B * H * W, N=Cin, K=k * k * Cout), Ho, Wo


def _nhwc(x, td, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(td).to(dev)


# ---- h2 tensors (geomapnet_amd/csrc/common.h): [..., C] fp32-class values as [..., C/32][hi | lo][32] fp16 ----------------
def h2_value(x):
    """the value an h2 tensor holds for x (fp32): hi + lo with hi = fp16(x), lo = fp16(x - hi)"""
    x = x.float()
    hi = x.to(torch.float16).float()
    return hi + (x - hi).to(torch.float16).float()


def to_h2(x):
    """fp32 [..., C] (C % 32 == 0) -> fp16 [..., 2C] in the pair layout"""
    x = x.float()
    Cc = x.shape[-1]
    assert Cc % 32 == 0
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    g = torch.stack([hi.reshape(*x.shape[:-1], Cc // 32, 32), lo.reshape(*x.shape[:-1], Cc // 32, 32)], dim=-2)
    return g.reshape(*x.shape[:-1], 2 * Cc).contiguous()


def from_h2(h):
    """fp16 [..., 2C] pair layout -> fp32 [..., C]"""
    Cc = h.shape[-1] // 2
    g = h.reshape(*h.shape[:-1], Cc // 32, 2, 32).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(*h.shape[:-1], Cc)


# ---- h2q tensors (geomapnet_amd/csrc/common.h): the h2 layout with fp8 planes behind the fp16 hi halves ----------------------------
QA_LO, QA_HI, QW_HI, QW_LO = 9, -1, 6, 16  # fixed exponents of the fp8 planes (common.h kQA_LO ...)


def _fp8(x, e):
    """fp8 e4m3 of x * 2^e, saturating; -> (uint8 codes, the values they stand for)"""
    q = (x.float() * 2.0 ** e).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), q.float() * 2.0 ** -e


def to_h2q(x, weight=False):
    """fp32 [..., C] (C % 32 == 0) -> (fp16 [..., 2C] buffer in the h2q layout, hi values, plane-0 values, plane-1 values): activation
    planes lo8 | hi8, weight planes hi8 | lo8"""
    x = x.float()
    Cc = x.shape[-1]
    assert Cc % 32 == 0
    hi = x.to(torch.float16)
    lo = x - hi.float()
    if weight:
        c0, v0 = _fp8(hi.float(), QW_HI)
        c1, v1 = _fp8(lo, QW_LO)
    else:
        c0, v0 = _fp8(lo, QA_LO)
        c1, v1 = _fp8(hi.float(), QA_HI)
    g = Cc // 32
    hib = hi.reshape(*x.shape[:-1], g, 32).contiguous().view(torch.uint8).reshape(*x.shape[:-1], g, 64)
    buf = torch.cat((hib, c0.reshape(*x.shape[:-1], g, 32), c1.reshape(*x.shape[:-1], g, 32)), dim=-1)  # [..., g, 128] bytes
    return buf.reshape(*x.shape[:-1], 4 * Cc).contiguous().view(torch.float16), hi.float(), v0, v1


def check_conv_fwd_h2q(lib, dev, B, H, W, Cin, Cout, k, stride, pad, seed=0):
    """h2q operands (dtype 5): hi*hi on the fp16 pipe + both cross terms from the fp8 planes in one scaled MFMA per K-step, against
    torch fp64 on EXACTLY the values the planes stand for (so the bar is accumulation rounding, not the fp8 approximation)"""
    _fresh()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, k, k, generator=gen) * (2.0 / (Cin * k * k)) ** 0.5
    xb, xhi, xlo8, xhi8 = to_h2q(x.permute(0, 2, 3, 1))
    wb, whi, whi8, wlo8 = to_h2q(w.permute(0, 2, 3, 1), weight=True)
    nchw = lambda t: t.permute(0, 3, 1, 2).double()  # noqa: E731
    ref = (F.conv2d(nchw(xhi), nchw(whi), stride=stride, padding=pad) + F.conv2d(nchw(xlo8), nchw(whi8), stride=stride, padding=pad) +
           F.conv2d(nchw(xhi8), nchw(wlo8), stride=stride, padding=pad))
    exact = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    g, Ho, Wo = fwd_geom(B, H, W, Cin, Cout, k, stride, pad)
    out = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float32, device=dev)
    st = torch.zeros(lib.op_igemm_grid_m(g.M), 2, Cout, device=dev)
    lib.check(lib.op_igemm(5, C.byref(g), K(xb.to(dev)), K(wb.to(dev)), K(out), Cout, K(st), None, 0, None, None, f32(1),
                           K(zero_page(dev)), None))
    dev_sync(dev)
    o = out.cpu().double().permute(0, 3, 1, 2)
    scale = ref.abs().max().item()
    err = (o - ref).abs().max().item()
    assert err <= 2e-5 * scale + 1e-6, (err, scale)
    approx = (o - exact).abs().max().item() / scale  # what the fp8 cross terms cost this product: ~2^-15 per term
    assert approx <= 2e-4, approx
    return err / scale, approx


def q_op(x, dtype):
    """x rounded to what a conv OPERAND of `dtype` holds (fp32 values)"""
    return h2_value(x) if dtype == 3 else x.to(TD[dtype]).float()


def up_op(x_last_c, dtype, dev):
    """upload a channels-last conv operand / gate in the storage form of `dtype`"""
    return (to_h2(x_last_c) if dtype == 3 else x_last_c.contiguous().to(TD[dtype])).to(dev)


def h2_hi(h):
    """the hi halves of an h2 tensor [..., 2C] as fp32 [..., C]: what a kernel that reads only those sees"""
    Cc = h.shape[-1] // 2
    return h.reshape(*h.shape[:-1], Cc // 32, 2, 32)[..., 0, :].float().reshape(*h.shape[:-1], Cc)


def gate_op(x_last_c, dtype, dev):
    """a ReLU gate (or another tensor of which a dtype-4 kernel reads the hi halves in place) -> (the values the kernel tests, the
    uploaded tensor).  dtype 4: relu(x) stored as h2 -- about half the entries exact zeros, lo halves with signs of their own --
    so a kernel that reads a lo half, another 32-channel group or a dense-row stride is wrong by O(1)"""
    if dtype == 4:
        h = to_h2(torch.relu(x_last_c.float()))
        return h2_hi(h), h.to(dev)
    q = q_op(x_last_c, dtype)
    return q, up_op(q, dtype, dev)


def check_conv_fwd(lib, dev, dtype, B, H, W, Cin, Cout, k, stride, pad, seed=0):
    _fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    x = q_op(torch.randn(B, Cin, H, W, generator=gen), dtype)
    w = q_op(torch.randn(Cout, Cin, k, k, generator=gen) * (2.0 / (Cin * k * k)) ** 0.5, dtype)
    ref = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    g, Ho, Wo = fwd_geom(B, H, W, Cin, Cout, k, stride, pad)
    xn, wn = up_op(x.permute(0, 2, 3, 1), dtype, dev), up_op(w.permute(0, 2, 3, 1), dtype, dev)
    out = torch.zeros(B, Ho, Wo, Cout, dtype=td, device=dev)
    gm = lib.op_igemm_grid_m(g.M)
    st = torch.zeros(gm, 2, Cout, device=dev)
    lib.check(lib.op_igemm(dtype, C.byref(g), K(xn), K(wn), K(out), Cout, K(st), None, 0, None, None, f32(1), K(zero_page(dev)), None))
    dev_sync(dev)
    o = out.cpu().double().permute(0, 3, 1, 2)
    scale = ref.abs().max().item()
    assert (o - ref).abs().max().item() <= OUT_TOL[dtype] * scale + 1e-6
    s1, s2 = st[:, 0].sum(0).cpu().double(), st[:, 1].sum(0).cpu().double()
    n = B * Ho * Wo
    assert (s1 - ref.sum((0, 2, 3))).abs().max().item() <= 1e-4 * scale * n ** 0.5 + 1e-4
    assert ((s2 - (ref ** 2).sum((0, 2, 3))).abs() / (ref ** 2).sum((0, 2, 3))).max().item() <= 1e-4


def check_conv_dgrad(lib, dev, dtype, B, H, W, Cin, Cout, k, stride, pad, with_res=True, seed=1):
    _fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    g, Ho, Wo = dgrad_geom(B, H, W, Cin, Cout, k, stride, pad)
    gy = q_op(torch.randn(B, Cout, Ho, Wo, generator=gen), dtype)
    w = q_op(torch.randn(Cout, Cin, k, k, generator=gen) * 0.1, dtype)
    x = torch.zeros(B, Cin, H, W, dtype=torch.double, requires_grad=True)
    F.conv2d(x, w.double(), stride=stride, padding=pad).backward(gy.double())
    want = x.grad.permute(0, 2, 3, 1)
    wt = up_op(w.permute(1, 2, 3, 0), dtype, dev)  # [Cin][R][S][Cout]
    res = gate = None
    if with_res:
        res = torch.randn(B, H, W, Cin, generator=gen).to(td)
        gate = q_op(torch.randn(B, H, W, Cin, generator=gen), dtype)
        want = want + torch.where(gate.double() > 0, res.double(), torch.zeros_like(res.double()))
        res, gate = res.to(dev), up_op(gate, dtype, dev)
    out = torch.zeros(B, H, W, Cin, dtype=td, device=dev)
    lib.check(lib.op_igemm(dtype, C.byref(g), K(up_op(gy.permute(0, 2, 3, 1), dtype, dev)), K(wt), K(out), Cin, None, None, 0, K(res),
                           K(gate), f32(1), K(zero_page(dev)), None))
    dev_sync(dev)
    assert (out.cpu().double() - want).abs().max().item() <= OUT_TOL[dtype] * want.abs().max().item() + 1e-6


def check_conv_dgrad_op(lib, dev, dtype, B, H, W, Cin, Cout, k, stride, pad, parity=1, mode="plain", seed=11):
    """conv-level data gradient (mn_op_conv_dgrad) vs autograd in fp64: generic form or parity classes of a stride-2
    conv, with the epilogue variants the training plan uses -- "plain"; "res_gate" (identity path, gated);
    "out_gate" (identity path + the gate of the block below applied to the stored sum); "inplace" (projection path
    accumulated in place: res is the output buffer, which for a 1x1 stride-2 conv leaves three quarters untouched)"""
    _fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gy = q_op(torch.randn(B, Cout, Ho, Wo, generator=gen), dtype)
    w = q_op(torch.randn(Cout, Cin, k, k, generator=gen) * 0.1, dtype)
    x = torch.zeros(B, Cin, H, W, dtype=torch.double, requires_grad=True)
    F.conv2d(x, w.double(), stride=stride, padding=pad).backward(gy.double())
    want = x.grad.permute(0, 2, 3, 1).contiguous()
    wt = up_op(w.permute(1, 2, 3, 0), dtype, dev)  # [Cin][R][S][Cout]
    out = torch.full((B, H, W, Cin), 7.0, dtype=td, device=dev)  # poison: every pixel must be written (or kept, in place)
    res = rgate = ogate = None
    if mode in ("res_gate", "out_gate", "inplace"):
        res = torch.randn(B, H, W, Cin, generator=gen).to(td)
        if mode == "res_gate":
            rgate, rgate_d = gate_op(torch.randn(B, H, W, Cin, generator=gen), dtype, dev)
            want = want + torch.where(rgate.double() > 0, res.double(), torch.zeros_like(res.double()))
            rgate = rgate_d
        else:
            want = want + res.double()
        if mode == "inplace":
            out = res.clone().to(dev)
            res = out
        else:
            res = res.to(dev)
    if mode in ("out_gate", "inplace"):
        ogate, ogate_d = gate_op(torch.randn(B, H, W, Cin, generator=gen), dtype, dev)
        if mode == "out_gate" or parity == 0 or k > 1:
            want = torch.where(ogate.double() > 0, want, torch.zeros_like(want))
        else:
            # 1x1 stride 2 by parity, in place: only the even pixels are visited (and gated); the others keep `res`
            m = torch.zeros(B, H, W, 1, dtype=torch.bool)
            m[:, ::2, ::2] = True
            want = torch.where(m & ~(ogate.double() > 0), torch.zeros_like(want), want)
        ogate = ogate_d
    lib.check(lib.op_conv_dgrad(dtype, B, H, W, Cin, Cout, k, stride, pad, K(up_op(gy.permute(0, 2, 3, 1), dtype, dev)), K(wt), K(out), K(res), K(rgate),
                                K(ogate), parity, K(zero_page(dev)), None))
    dev_sync(dev)
    err = (out.cpu().double() - want).abs().max().item()
    assert err <= OUT_TOL[1 if dtype == 4 else dtype] * want.abs().max().item() + 1e-6, err


def check_conv_halo_h2(lib, dev, B, H, W, seed=23, stats=True):
    """csrc/halo_h2.h: the 64 -> 64 channel 3x3 forward convolution of h2 tensors with the weights in registers (layer1 of the fp16x2 /
    fp16x2m modes) vs torch fp64 on exactly the values the h2 operands stand for: fp32 output to the h2 kernels' tolerance, BatchNorm
    column sums; ragged tiles (H, W not multiples of 8 / 16) exercise the out-of-image masks and the zero-filled halo"""
    _fresh()
    gen = torch.Generator().manual_seed(seed)
    x = h2_value(torch.randn(B, 64, H, W, generator=gen))
    w = h2_value(torch.randn(64, 64, 3, 3, generator=gen) * (2.0 / (64 * 9)) ** 0.5)
    ref = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    g, Ho, Wo = fwd_geom(B, H, W, 64, 64, 3, 1, 1)
    xn, wn = to_h2(x.permute(0, 2, 3, 1)).to(dev), to_h2(w.permute(0, 2, 3, 1).reshape(64, 9 * 64)).to(dev)
    out = torch.full((B, H, W, 64), 7.0, dtype=torch.float32, device=dev)
    st = torch.zeros(5, 2, 64, device=dev, dtype=torch.double) if stats else None
    lib.check(lib.op_conv_halo_h2(C.byref(g), K(xn), K(wn), K(out), 64, K(st), 5, None))
    dev_sync(dev)
    scale = ref.abs().max().item()
    err = (out.cpu().double() - ref).abs().max().item()
    assert err <= OUT_TOL[3] * scale + 1e-6, err
    if st is not None:
        sums = st.cpu().double().sum(0)
        r2 = ref.reshape(-1, 64)
        assert (sums[0] - r2.sum(0)).abs().max().item() <= 1e-4 * scale * r2.shape[0] ** 0.5 + 1e-4
        assert ((sums[1] - (r2 ** 2).sum(0)).abs() / (r2 ** 2).sum(0)).max().item() <= 1e-4
    return err / scale


def check_conv_halo(lib, dev, B, H, W, Cout=64, dgrad=False, mode="plain", seed=21, pp_wgs=0, gate_h2=False):
    """fp16 3x3 stride-1 convolution of 64 -> 64 channels from an LDS-resident halo tile, persistent two-group kernel
    (csrc/halo_pp.h) vs torch fp64: forward (with BatchNorm column sums) or data gradient, epilogue variants as
    check_conv_dgrad_op; ragged tiles (H, W not multiples of 16) exercise the out-of-image masks.  pp_wgs: number of
    workgroups (0 = one per CU); fewer workgroups than tiles walks the phase loop.  gate_h2: the gates are h2 tensors of which the
    hi halves are read (mn_op_conv_halo_pp_h2gates: the fp16x2m mode's layer1 data gradients)"""
    _fresh()
    td, Cin, k = torch.float16, 64, 3
    gdt = 4 if gate_h2 else 1
    gen = torch.Generator().manual_seed(seed)
    if not dgrad:
        g, Ho, Wo = fwd_geom(B, H, W, Cin, Cout, k, 1, 1)
        x = torch.randn(B, Cin, H, W, generator=gen).to(td).float()
        w = (torch.randn(Cout, Cin, k, k, generator=gen) * 0.1).to(td).float()
        want = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
        a = _nhwc(x, td, dev)
        bw = w.permute(0, 2, 3, 1).contiguous().to(td).to(dev)  # [Cout][R][S][Cin]
        N = Cout
    else:
        # data gradient of a conv with `Cout` output channels and 64 INPUT channels would have C = Cout; the kernel
        # needs C = 64, so the gradient case is conv(Cx -> 64): gy has 64 channels, gx has Cout channels
        g, Ho, Wo = dgrad_geom(B, H, W, Cout, 64, k, 1, 1)
        gy = torch.randn(B, 64, H, W, generator=gen).to(td).float()
        w = (torch.randn(64, Cout, k, k, generator=gen) * 0.1).to(td).float()
        xin = torch.zeros(B, Cout, H, W, dtype=torch.double, requires_grad=True)
        F.conv2d(xin, w.double(), padding=1).backward(gy.double())
        want = xin.grad.permute(0, 2, 3, 1).contiguous()
        a = _nhwc(gy, td, dev)
        bw = w.permute(1, 2, 3, 0).contiguous().to(td).to(dev)  # [Cin][R][S][Cout]
        N = Cout
    res = rgate = ogate = None
    if mode in ("res_gate", "out_gate"):
        res = torch.randn(B, H, W, N, generator=gen).to(td)
        if mode == "res_gate":
            rgate, rgate_d = gate_op(torch.randn(B, H, W, N, generator=gen), gdt, dev)
            want = want + torch.where(rgate.double() > 0, res.double(), torch.zeros_like(res.double()))
            rgate = rgate_d
        else:
            want = want + res.double()
            ogate, ogate_d = gate_op(torch.randn(B, H, W, N, generator=gen), gdt, dev)
            want = torch.where(ogate.double() > 0, want, torch.zeros_like(want))
            ogate = ogate_d
        res = res.to(dev)
    out = torch.full((B, H, W, N), 7.0, dtype=td, device=dev)
    st = torch.zeros(5, 2, N, device=dev, dtype=torch.double) if not dgrad else None
    op = lib.op_conv_halo_pp_h2gates if gate_h2 else lib.op_conv_halo_pp
    lib.check(op(C.byref(g), K(a), K(bw), K(out), N, K(st), 5, 0, K(res), K(rgate), K(ogate), f32(1), pp_wgs, None))
    dev_sync(dev)
    err = (out.cpu().double() - want).abs().max().item()
    assert err <= OUT_TOL[1] * want.abs().max().item() + 1e-6, err
    if st is not None:
        sums = st.cpu().double().sum(0)
        ref = want.reshape(-1, N)
        assert (sums[0] - ref.sum(0)).abs().max().item() <= 2e-3 * ref.abs().sum(0).max().item()
        assert (sums[1] - (ref * ref).sum(0)).abs().max().item() <= 2e-3 * (ref * ref).sum(0).max().item()


def check_conv_wgrad(lib, dev, dtype, B, H, W, Cin, Cout, k, stride, pad, target_blocks=8, seed=2, ws=False):
    _fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    g, Ho, Wo = fwd_geom(B, H, W, Cin, Cout, k, stride, pad)
    gy = q_op(torch.randn(B, Cout, Ho, Wo, generator=gen), dtype)
    gyn = up_op(gy.permute(0, 2, 3, 1), dtype, dev)
    if dtype == 4:  # X: an h2 activation (relu) of which the kernel reads the hi halves in place; the reference contracts those
        x, xn = gate_op(torch.randn(B, Cin, H, W, generator=gen).permute(0, 2, 3, 1), dtype, dev)
        x = x.permute(0, 3, 1, 2)
    else:
        x = q_op(torch.randn(B, Cin, H, W, generator=gen), dtype)
        xn = up_op(x.permute(0, 2, 3, 1), dtype, dev)
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.double, requires_grad=True)
    F.conv2d(x.double(), w, stride=stride, padding=pad).backward(gy.double())
    ref = w.grad.permute(0, 2, 3, 1).reshape(Cout, -1)
    dW = torch.zeros(Cout, k * k * Cin, device=dev)
    if ws:  # partial tiles through a workspace + ordered reduction (the plan's form), twice: results must be bit-identical
        wsf = int(lib.op_wgrad_ws_floats())
        wbuf = torch.full((wsf,), float("nan"), device=dev)
        dW2 = torch.zeros_like(dW)
        for out in (dW, dW2):
            lib.check(lib.op_wgrad_ws(dtype, C.byref(g), K(gyn), Cout, K(xn), K(out), k * k * Cin,
                                      f32(0.5), K(wbuf), wsf, K(zero_page(dev)), None))
        dev_sync(dev)
        if dtype in (1, 2, 3, 4) and k == 3 and stride == 1 and Cout * 9 * Cin // 4 >= 131072:
            assert torch.equal(dW, dW2)  # one reduction group: chunks are summed in index order, no atomics anywhere
    else:
        lib.check(lib.op_wgrad(dtype, C.byref(g), K(gyn), Cout, K(xn), K(dW), k * k * Cin,
                               None, f32(0.5), target_blocks, K(zero_page(dev)), None))
    dev_sync(dev)
    assert (dW.cpu().double() - 0.5 * ref).abs().max().item() <= 2e-5 * ref.abs().max().item() * max(1, (B * Ho * Wo) ** 0.5 / 8)


def stem_geom(B, H, W):
    """the plan's stem: 7x7/2 pad 3 conv as a 7x4 conv over pixel pairs of the zero-padded NHWC4 image"""
    Hp, Wp = H + 6, (W + 8) & ~1
    H0, W0 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = GatherGeom(B=B, Hi=Hp, Wi=Wp // 2, C=8, P=H0, Q=W0, R=7, S=4, mul_p=2, mul_q=1, rsign=1, ssign=1, off_h=0, off_w=0,
                   div=1, M=B * H0 * W0, N=64, K=224)
    return g, Hp, Wp, H0, W0


def check_stem(lib, dev, dtype, B, H, W, seed=3):
    """stem forward + weight gradient through the padded pixel-pair formulation vs conv2d(7,2,3)"""
    _fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=gen).to(td).float()
    w = (torch.randn(64, 3, 7, 7, generator=gen) * 0.1).to(td).float()
    g, Hp, Wp, H0, W0 = stem_geom(B, H, W)
    xp = torch.zeros(B, Hp, Wp, 4)
    xp[:, 3:3 + H, 3:3 + W, :3] = x.permute(0, 2, 3, 1)
    wc = torch.zeros(64, 7, 8, 4)
    wc[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    wd = w.double().clone().requires_grad_(True)
    ref = F.conv2d(x.double(), wd, stride=2, padding=3)
    assert ref.shape[2] == H0 and ref.shape[3] == W0
    out = torch.zeros(B, H0, W0, 64, dtype=td, device=dev)
    lib.check(lib.op_igemm(dtype, C.byref(g), K(xp.to(td).to(dev)), K(wc.reshape(64, 224).to(td).to(dev)), K(out), 64,
                           None, None, 0, None, None, f32(1), K(zero_page(dev)), None))
    dev_sync(dev)
    assert (out.cpu().double().permute(0, 3, 1, 2) - ref).abs().max().item() <= OUT_TOL[dtype] * ref.abs().max().item()
    if dtype == 1:  # the dedicated stem kernel (weights in registers, pixel pairs straight from LDS) + its BatchNorm sums
        out2 = torch.full((B, H0, W0, 64), float("nan"), dtype=td, device=dev)
        acc = torch.zeros(3, 2, 64, dtype=torch.float64, device=dev)
        lib.check(lib.op_stem_conv(K(xp.to(td).to(dev)), K(wc.reshape(64, 224).to(td).to(dev)), K(out2), K(acc), 3, B, H, W, Wp, None))
        dev_sync(dev)
        o2 = out2.cpu().double().permute(0, 3, 1, 2)
        assert (o2 - ref).abs().max().item() <= OUT_TOL[dtype] * ref.abs().max().item()
        n = B * H0 * W0
        rd = ref.detach()
        s1, s2 = acc[:, 0].sum(0).cpu(), acc[:, 1].sum(0).cpu()
        assert (s1 - rd.sum((0, 2, 3))).abs().max().item() <= 1e-4 * rd.abs().max().item() * n ** 0.5 + 1e-4
        assert ((s2 - (rd ** 2).sum((0, 2, 3))).abs() / (rd ** 2).sum((0, 2, 3))).max().item() <= 1e-4
    if dtype == 2:  # the split-operand form of the stem kernel (fp32 tensors, the fp32x3 / fp16x2 modes' stem) + its sums
        out2 = torch.full((B, H0, W0, 64), float("nan"), device=dev)
        acc = torch.zeros(3, 2, 64, dtype=torch.float64, device=dev)
        lib.check(lib.op_stem_conv_x3(K(xp.to(dev)), K(wc.reshape(64, 224).to(dev)), K(out2), K(acc), 3, B, H, W, Wp, None))
        dev_sync(dev)
        o2 = out2.cpu().double().permute(0, 3, 1, 2)
        assert (o2 - ref).abs().max().item() <= OUT_TOL[dtype] * ref.abs().max().item()
        n = B * H0 * W0
        rd = ref.detach()
        s1, s2 = acc[:, 0].sum(0).cpu(), acc[:, 1].sum(0).cpu()
        assert (s1 - rd.sum((0, 2, 3))).abs().max().item() <= 1e-4 * rd.abs().max().item() * n ** 0.5 + 1e-4
        assert ((s2 - (rd ** 2).sum((0, 2, 3))).abs() / (rd ** 2).sum((0, 2, 3))).max().item() <= 1e-4
    gy = torch.randn(B, 64, H0, W0, generator=gen).to(td).float()
    ref.backward(gy.double())
    cm = torch.full((224,), -1, dtype=torch.int32)
    for r in range(7):
        for s4 in range(4):
            for e in range(8):
                sp, ch = 2 * s4 + (e >> 2), e & 3
                if sp < 7 and ch < 3:
                    cm[(r * 4 + s4) * 8 + e] = (r * 7 + sp) * 3 + ch
    dW = torch.zeros(64, 147, device=dev)
    lib.check(lib.op_wgrad(dtype, C.byref(g), K(_nhwc(gy, td, dev)), 64, K(xp.to(td).to(dev)), K(dW), 147,
                           K(cm.to(dev)), f32(1), 16, K(zero_page(dev)), None))
    dev_sync(dev)
    want = wd.grad.permute(0, 2, 3, 1).reshape(64, 147)
    assert (dW.cpu().double() - want).abs().max().item() <= 1e-4 * want.abs().max().item()


def check_bn(lib, dev, dtype, M, Cc, relu=True, with_res=True, gate=True, seed=4):
    """training-mode BatchNorm forward (+residual, ReLU) and backward vs torch autograd in fp64"""
    _fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    y = (torch.randn(M, Cc, generator=gen) * 1.5 + 0.3).to(td)
    res = torch.randn(M, Cc, generator=gen).to(td) if with_res else None
    gamma, beta = torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen)
    rm, rv = torch.zeros(Cc), torch.ones(Cc)
    yd = y.double().clone().requires_grad_(True)
    gd, bd = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    rmd, rvd = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(yd, rmd, rvd, gd, bd, training=True, momentum=0.1, eps=1e-5)
    if with_res:
        z = z + res.double()
    o_ref = F.relu(z) if relu else z
    mean, invstd = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
    out = torch.zeros(M, Cc, dtype=td, device=dev)
    scratch = torch.zeros(2 * Cc * 8 + 2 * Cc * 4, dtype=torch.uint8, device=dev)
    rm_d, rv_d = rm.to(dev), rv.to(dev)
    yv = y.to(dev)
    lib.check(lib.op_bn_train_fwd(dtype, K(yv), M, Cc, K(gamma.to(dev)), K(beta.to(dev)), K(rm_d), K(rv_d), K(mean),
                                  K(invstd), K(res.to(dev)) if with_res else None, int(relu), K(out), f32(1e-5), f32(0.1),
                                  K(scratch), None))
    dev_sync(dev)
    tol = OUT_TOL[dtype] * o_ref.abs().max().item() + 1e-5
    assert (out.cpu().double() - o_ref).abs().max().item() <= tol
    np.testing.assert_allclose(rm_d.cpu().numpy(), rmd.numpy(), atol=1e-5)
    np.testing.assert_allclose(rv_d.cpu().numpy(), rvd.numpy(), rtol=1e-5, atol=1e-5)
    # backward with the device's own stored output as ReLU gate
    g_out = torch.randn(M, Cc, generator=gen).to(td)
    outq = out.cpu().double()
    gm = g_out.double() * (outq > 0).double() if (relu and gate) else g_out.double()
    z2 = F.batch_norm(yd, rmd.clone(), rvd.clone(), gd, bd, training=True, momentum=0.1, eps=1e-5)
    z2.backward(gm)
    dgamma, dbeta = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
    gy = torch.zeros(M, Cc, dtype=td, device=dev)
    coef = torch.zeros(3 * Cc, device=dev)
    acc = torch.zeros(2 * Cc, dtype=torch.float64, device=dev)
    lib.check(lib.op_bn_bwd(dtype, K(g_out.to(dev)), K(out) if (relu and gate) else None, K(yv), M, Cc, K(gamma.to(dev)),
                            K(mean), K(invstd), K(dgamma), K(dbeta), K(gy), K(coef), K(acc), f32(1.0), None))
    dev_sync(dev)
    assert (gy.cpu().double() - yd.grad).abs().max().item() <= OUT_TOL[dtype] * yd.grad.abs().max().item() * 2 + 1e-6
    np.testing.assert_allclose(dgamma.cpu().numpy(), gd.grad.numpy(), rtol=2e-4, atol=2e-4 * M ** 0.5)
    np.testing.assert_allclose(dbeta.cpu().numpy(), bd.grad.numpy(), rtol=2e-4, atol=2e-4 * M ** 0.5)
    assert float(acc.abs().max()) == 0.0  # accumulators are handed back zeroed


def check_maxpool(lib, dev, dtype, B, H, W, Cc, seed=5, ties=False):
    _fresh()
    td = TD[dtype]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cc, H, W, generator=gen)
    if ties:
        x = torch.relu(x).round()  # many equal values and zeros: first-max routing matters
    x = x.to(td).float()
    xd = x.double().clone().requires_grad_(True)
    ref = F.max_pool2d(xd, 3, 2, 1)
    Po, Qo = ref.shape[2], ref.shape[3]
    xn = _nhwc(x, td, dev)
    out = torch.zeros(B, Po, Qo, Cc, dtype=td, device=dev)
    idx = torch.zeros(B, Po, Qo, Cc, dtype=torch.uint8, device=dev)
    lib.check(lib.op_maxpool_fwd(dtype, K(xn), K(out), K(idx), B, H, W, Cc, None))
    dev_sync(dev)
    assert torch.equal(out.cpu().double().permute(0, 3, 1, 2), ref.detach())
    go = torch.randn(B, Cc, Po, Qo, generator=gen).to(td).float()
    ref.backward(go.double())
    gin = torch.zeros(B, H, W, Cc, dtype=td, device=dev)
    lib.check(lib.op_maxpool_bwd(dtype, K(idx), K(_nhwc(go, td, dev)), K(gin), B, H, W, Cc, None))
    dev_sync(dev)
    want = xd.grad.permute(0, 2, 3, 1)
    assert (gin.cpu().double() - want).abs().max().item() <= OUT_TOL[dtype] * max(1.0, want.abs().max().item())


# ---- the h2 / record BatchNorm of the fp16x2 / fp16x2m modes (csrc/elementwise_h2.h) -----------------------------------------
REC_RTOL, REC_ATOL = 1.5 * 2.0 ** -10, 1e-6  # record: fp16 round-to-nearest (2^-11) + the lowest mantissa bit cleared (<= 2^-10)


def rec_decode(rec):
    """2-byte backward record -> (xhat it stands for as fp64, gate bit as bool)"""
    bits = rec.cpu().contiguous().view(torch.int16)
    return (bits & -2).view(torch.float16).double(), (bits & 1) != 0


def _bn_inputs(M, Cc, seed):
    """check_bn's input distribution, fp32"""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(M, Cc, generator=gen) * 1.5 + 0.3
    res = torch.randn(M, Cc, generator=gen)
    gamma, beta = torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen)
    return gen, y, res, gamma, beta


def check_bn_h2_forward(lib, dev, M, Cc, seed=4):
    """mn_op_bn_train_fwd_h2 (statistics, finalize, bn_apply_h2_kernel) in the variants the plan uses -- (relu, res) = (1, none),
    (0, none), (1, h2 res), each with and without the backward record -- against the fp64 BatchNorm of the fp32 y plus the value the
    h2 residual holds: output at OUT_TOL[3], running statistics as check_bn, every record element inside REC_RTOL / REC_ATOL of the
    fp64 xhat, gate bits EXACTLY (out > 0) for relu without residual and 1 everywhere else; out and rec are NaN-filled before the
    launch.  Returns what check_bn_rec_backward needs: the records of (1, none) and (0, none) as the device wrote them."""
    _fresh()
    gen, y, res, gamma, beta = _bn_inputs(M, Cc, seed)
    res_h = to_h2(res)
    yd = y.double()
    rmd, rvd = torch.zeros(Cc, dtype=torch.double), torch.ones(Cc, dtype=torch.double)
    z = F.batch_norm(yd, rmd, rvd, gamma.double(), beta.double(), training=True, momentum=0.1, eps=1e-5)
    mean64, var64 = yd.mean(0), yd.var(0, unbiased=False)
    xhat64 = (yd - mean64) / torch.sqrt(var64 + 1e-5)
    # a pre-activation in (0, 2^-24) would be positive for the gate while both halves of the stored output flush to zero
    assert not ((z > 0) & (z < 2.0 ** -24)).any(), "input has a pre-activation inside (0, 2^-24)"
    yv, gam_d, bet_d, res_d = y.to(dev), gamma.to(dev), beta.to(dev), res_h.to(dev)
    recs = {}
    for relu, with_res in ((1, False), (0, False), (1, True)):
        o_ref = z + from_h2(res_h).double() if with_res else z
        if relu:
            o_ref = F.relu(o_ref)
        for with_rec in (True, False):
            mean, invstd = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
            out = torch.full((M, 2 * Cc), float("nan"), dtype=torch.float16, device=dev)
            rec = torch.full((M, Cc), float("nan"), dtype=torch.float16, device=dev) if with_rec else None
            scratch = torch.zeros(2 * Cc * 8 + 2 * Cc * 4, dtype=torch.uint8, device=dev)
            rm_d, rv_d = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
            lib.check(lib.op_bn_train_fwd_h2(K(yv), M, Cc, K(gam_d), K(bet_d), K(rm_d), K(rv_d), K(mean), K(invstd),
                                             K(res_d) if with_res else None, relu, K(out), K(rec), f32(1e-5), f32(0.1), K(scratch), None))
            dev_sync(dev)
            oh = out.cpu()
            assert not torch.isnan(oh).any()  # every hi and lo half written
            o = from_h2(oh).double()
            err = (o - o_ref).abs().max().item()
            assert err <= OUT_TOL[3] * o_ref.abs().max().item() + 1e-5, (relu, with_res, err)
            np.testing.assert_allclose(rm_d.cpu().numpy(), rmd.numpy(), atol=1e-5)
            np.testing.assert_allclose(rv_d.cpu().numpy(), rvd.numpy(), rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(mean.cpu().numpy(), mean64.numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(invstd.cpu().numpy(), (1.0 / torch.sqrt(var64 + 1e-5)).numpy(), rtol=1e-5)
            if not with_rec:
                continue
            assert not torch.isnan(rec.cpu()).any()
            xh, gate = rec_decode(rec)
            ratio = ((xh - xhat64).abs() / (REC_RTOL * xhat64.abs() + REC_ATOL)).max().item()
            assert ratio <= 1.0, ("record / bound", relu, with_res, ratio)
            if relu and not with_res:
                assert torch.equal(gate, o > 0)
            else:
                assert gate.all()
            if not with_res:
                recs[relu] = rec
    return dict(M=M, C=Cc, gen=gen, y=y, gamma=gamma, beta=beta, mean=mean, invstd=invstd, recs=recs, xhat64=xhat64)


def check_bn_rec_backward(lib, dev, fwd, grad_unscale=0.25):
    """BatchNorm backward from the record (mn_op_bn_bwd_rows dtype 4: bn_bwd_reduce_rec_kernel<4>, bn_finalize_bwd_kernel,
    bn_bwd_apply_rec_kernel) on the records check_bn_h2_forward's launches wrote.
    (1) against fp64 on the operands as stored -- xhat := the decoded record, gm := g * gate bit (use_gate) or g, k1 = gamma * the
    device's invstd: gy = k1 (gm - mean(gm) - xhat mean(gm xhat)), dbeta = sum gm, dgamma = sum gm xhat (the closed form of autograd's
    BatchNorm backward; asserted equal to autograd in (2)) -- at check_bn's fp16 bars; accumulators come back zeroed; accum_rows 1 and 4.
    (2) against autograd in fp64 through batch_norm(y) itself.  With xh = xhat (1 + d), |d| <= r = REC_RTOL (+ REC_ATOL absolute),
        gy_rec - gy_true = -k1 [ (xh - xhat) mgx' + xhat (mgx' - mgx) ],  mgx = mean(gm xhat), mgx' = mean(gm xh).
    First term: <= r |k1| |mgx'| |xhat|, the record bound propagated.  Second term: mgx' - mgx = mean(gm xhat d) averages M signed
    rounding errors; even its worst case r mean|gm xhat| (~0.6 r for these inputs) times |k1| max|xhat| (~4.5) stays below the fp16
    output bar 2 OUT_TOL[1] max|gy| (max|gy| ~ 4 |k1|) that (1) grants the stored gradient, so it is not given a term of its own.
    Bound per element: r |k1| |mgx| |xhat| + 2 OUT_TOL[1] max|gy| + 1e-6."""
    M, Cc, y, gamma = fwd["M"], fwd["C"], fwd["y"], fwd["gamma"]
    g = torch.randn(M, Cc, generator=fwd["gen"]).to(torch.float16)
    g64 = g.double()
    invstd_d = fwd["invstd"].cpu().double()
    k1 = gamma.double() * invstd_d
    g_d, gam_d = g.to(dev), gamma.to(dev)
    for relu, use_gate, rows in ((1, True, 1), (1, True, 4), (1, False, 1), (0, True, 4)):
        rec = fwd["recs"][relu]
        xh, gate = rec_decode(rec)
        gm = g64 * gate.double() if use_gate else g64
        mg, mgx = gm.mean(0), (gm * xh).mean(0)
        gy_ref = k1 * (gm - mg - xh * mgx)
        dgamma, dbeta = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
        gy = torch.full((M, Cc), float("nan"), dtype=torch.float16, device=dev)
        coef = torch.zeros(4 * Cc, device=dev)
        acc = torch.full((rows * 2 * Cc,), 3.0, dtype=torch.float64, device=dev)  # (the operator zeroes its scratch on entry too)
        lib.check(lib.op_bn_bwd_rows(4, K(g_d), K(g_d) if use_gate else None, K(rec), M, Cc, K(gam_d), None, K(fwd["mean"]),
                                     K(fwd["invstd"]), K(dgamma), K(dbeta), K(gy), K(coef), K(acc), rows, f32(grad_unscale), None))
        dev_sync(dev)
        got = gy.cpu().double()
        out_tol = OUT_TOL[1] * gy_ref.abs().max().item() * 2 + 1e-6
        err = (got - gy_ref).abs().max().item()
        assert err <= out_tol, ("gy vs the decoded record", relu, use_gate, rows, err, out_tol)
        # (grad_unscale is a power of two: dividing it out is exact, the bars are check_bn's)
        np.testing.assert_allclose(dgamma.cpu().numpy() / grad_unscale, (gm * xh).sum(0).numpy(), rtol=2e-4, atol=2e-4 * M ** 0.5)
        np.testing.assert_allclose(dbeta.cpu().numpy() / grad_unscale, gm.sum(0).numpy(), rtol=2e-4, atol=2e-4 * M ** 0.5)
        assert float(acc.abs().max()) == 0.0  # accumulators are handed back zeroed
        # (2) the true backward pass
        yd = y.double().clone().requires_grad_(True)
        F.batch_norm(yd, None, None, gamma.double(), None, True, 0.0, 1e-5).backward(gm)
        xhat = fwd["xhat64"]
        k1t = gamma.double() / torch.sqrt(y.double().var(0, unbiased=False) + 1e-5)
        closed = k1t * (gm - mg - xhat * (gm * xhat).mean(0))
        assert (closed - yd.grad).abs().max().item() <= 1e-9 * max(1.0, yd.grad.abs().max().item())
        bound = REC_RTOL * k1.abs() * (gm * xhat).mean(0).abs() * xhat.abs() + OUT_TOL[1] * yd.grad.abs().max().item() * 2 + 1e-6
        worst = ((got - yd.grad).abs() / bound).max().item()
        assert worst <= 1.0, ("gy vs the true backward / bound", relu, use_gate, rows, worst)


def check_bn_h2_backward(lib, dev, M, Cc, self_gate, rows=1, seed=4, grad_unscale=0.5):
    """launch_bn_bwd_h2 (mn_op_bn_bwd / mn_op_bn_bwd_rows dtype 3: fp32 g and y in, h2 d(conv output) out, the gate none or the unit's
    own ReLU recomputed from y) vs torch autograd in fp64 at OUT_TOL[3] and check_bn's bars for d(gamma), d(beta).  The kernel
    recomputes the gate in fp32, so the input is first moved off the threshold: a y whose pre-activation lies within 1e-3 of zero is
    pushed 0.01 / k1 away (the statistics move by O(1e-6)), and the check asserts that none is left within 1e-4."""
    _fresh()
    gen, y, _, gamma, beta = _bn_inputs(M, Cc, seed)

    def stats(y):
        yd = y.double()
        mean, var = yd.mean(0), yd.var(0, unbiased=False)
        return mean.float(), (1.0 / torch.sqrt(var + 1e-5)).float()
    mean, invstd = stats(y)
    z = (y.double() - mean.double()) * (gamma.double() * invstd.double()) + beta.double()
    y = torch.where(z.abs() < 1e-3, y + (0.01 / (gamma * invstd)) * torch.where(z >= 0, 1.0, -1.0), y).float()
    mean, invstd = stats(y)
    z = (y.double() - mean.double()) * (gamma.double() * invstd.double()) + beta.double()
    assert z.abs().min().item() > 1e-4
    g = torch.randn(M, Cc, generator=gen)
    gm = g.double() * (z > 0).double() if self_gate else g.double()
    yd = y.double().clone().requires_grad_(True)
    gd = gamma.double().clone().requires_grad_(True)
    bd = beta.double().clone().requires_grad_(True)
    F.batch_norm(yd, None, None, gd, bd, True, 0.0, 1e-5).backward(gm)
    dgamma, dbeta = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
    gy = torch.full((M, 2 * Cc), float("nan"), dtype=torch.float16, device=dev)
    coef = torch.zeros(4 * Cc, device=dev)
    acc = torch.full((rows * 2 * Cc,), 3.0, dtype=torch.float64, device=dev)
    args = (K(g.to(dev)), None, K(y.to(dev)), M, Cc, K(gamma.to(dev)))
    tail = (K(mean.to(dev)), K(invstd.to(dev)), K(dgamma), K(dbeta), K(gy), K(coef), K(acc))
    if self_gate or rows != 1:
        lib.check(lib.op_bn_bwd_rows(3, *args, K(beta.to(dev)) if self_gate else None, *tail, rows, f32(grad_unscale), None))
    else:
        lib.check(lib.op_bn_bwd(3, *args, *tail, f32(grad_unscale), None))
    dev_sync(dev)
    gh = gy.cpu()
    assert not torch.isnan(gh).any()
    err = (from_h2(gh).double() - yd.grad).abs().max().item()
    assert err <= OUT_TOL[3] * yd.grad.abs().max().item() * 2 + 1e-6, err
    np.testing.assert_allclose(dgamma.cpu().numpy() / grad_unscale, gd.grad.numpy(), rtol=2e-4, atol=2e-4 * M ** 0.5)
    np.testing.assert_allclose(dbeta.cpu().numpy() / grad_unscale, bd.grad.numpy(), rtol=2e-4, atol=2e-4 * M ** 0.5)
    assert float(acc.abs().max()) == 0.0


def check_bn_dtype_errors(lib, dev):
    """dtype / channel combinations the BatchNorm entries do not have fail with a message instead of running another path"""
    _fresh()
    t = torch.zeros(64 * 64, device=dev)
    a = K(t)
    for dt in (3, 4, 5, 7):
        assert lib.op_bn_train_fwd(dt, a, 8, 64, a, a, a, a, a, a, None, 1, a, f32(1e-5), f32(0.1), a, None) != 0
        assert b"dtype" in lib.last_error()
    assert lib.op_bn_bwd(5, a, None, a, 8, 64, a, a, a, a, a, a, a, a, f32(1.0), None) != 0
    assert lib.op_bn_bwd(3, a, a, a, 8, 64, a, a, a, a, a, a, a, a, f32(1.0), None) != 0  # fp16x2 has no gate tensor
    for dt in (3, 4):
        assert lib.op_bn_bwd(dt, a, None, a, 8, 48, a, a, a, a, a, a, a, a, f32(1.0), None) != 0  # C not 32 .. 512, a power of two
        assert b"bn:" in lib.last_error()
    assert lib.op_bn_train_fwd_h2(a, 8, 16, a, a, a, a, a, a, None, 1, a, None, f32(1e-5), f32(0.1), a, None) != 0
    assert lib.op_bn_bwd_rows(4, a, None, a, 8, 64, a, None, a, a, a, a, a, a, a, 0, f32(1.0), None) != 0  # accum_rows < 1
    assert lib.op_avgpool_bwd(1, a, a, None, 1, 4, 64, None) != 0
    assert lib.op_avgpool_fwd_h2(a, a, 1, 4, 48, None) != 0
    assert lib.op_widen_f16(a, a, 12, None) != 0
    g, _, _ = fwd_geom(1, 4, 4, 48, 64, 3, 1, 1)
    assert lib.op_wgrad(4, C.byref(g), a, 64, a, a, 9 * 48, None, f32(1.0), 1, K(zero_page(dev)), None) != 0  # h2 X: C % 32
    assert lib.op_wgrad(5, C.byref(g), a, 64, a, a, 9 * 48, None, f32(1.0), 1, K(zero_page(dev)), None) != 0
    assert lib.op_conv_dgrad(5, 1, 4, 4, 64, 64, 3, 1, 1, a, a, a, None, None, None, 1, K(zero_page(dev)), None) != 0
    assert lib.op_conv_dgrad(4, 1, 4, 4, 48, 64, 3, 1, 1, a, a, a, None, None, a, 1, K(zero_page(dev)), None) != 0  # h2 gate: Cin % 32


def check_stem_pool_h2(lib, dev, B, H0, W0, exact=True, seed=5):
    """bn_relu_maxpool_h2_kernel (mn_op_bn_relu_maxpool_h2: the stem's BatchNorm + ReLU + 3x3/2 max-pool of the fp16x2 / fp16x2m modes,
    coefficients given directly) vs torch fp64.  exact: power-of-two scales, dyadic shifts and small-integer y make the fp32
    arithmetic exact and ties / zeros plentiful (as check_maxpool's ties=True): the pooled h2 value EQUALS the reference, the argmax
    bytes route a gradient through mn_op_maxpool_bwd exactly as autograd does (first maximum wins), and y16 -- NaN-filled
    beforehand -- equals fp16(y) everywhere.  Otherwise random y / coefficients: pooled value at OUT_TOL[3], y16 bit for bit."""
    _fresh()
    Cc = 64
    gen = torch.Generator().manual_seed(seed)
    if exact:
        y = (torch.randn(B, H0, W0, Cc, generator=gen) * 2).round()
        scale = 2.0 ** torch.randint(-2, 2, (Cc,), generator=gen).float() * torch.where(torch.rand(Cc, generator=gen) < 0.25, -1.0, 1.0)
        shift = torch.randint(-8, 9, (Cc,), generator=gen).float() / 4
    else:
        y = torch.randn(B, H0, W0, Cc, generator=gen) * 1.5 + 0.3
        scale = (torch.rand(Cc, generator=gen) + 0.5) * torch.where(torch.rand(Cc, generator=gen) < 0.25, -1.0, 1.0)
        shift = torch.randn(Cc, generator=gen)
    a = F.relu(y.double() * scale.double() + shift.double()).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = F.max_pool2d(a, 3, 2, 1)
    Po, Qo = ref.shape[2], ref.shape[3]
    out = torch.full((B, Po, Qo, 2 * Cc), float("nan"), dtype=torch.float16, device=dev)
    idx = torch.full((B, Po, Qo, Cc), 255, dtype=torch.uint8, device=dev)
    y16 = torch.full((B, H0, W0, Cc), float("nan"), dtype=torch.float16, device=dev)
    coef = torch.cat((scale, shift)).to(dev)
    lib.check(lib.op_bn_relu_maxpool_h2(K(y.to(dev)), K(coef), K(out), K(idx), K(y16), B, H0, W0, Cc, None))
    dev_sync(dev)
    oh = out.cpu()
    assert not torch.isnan(oh).any()
    o = from_h2(oh).double().permute(0, 3, 1, 2)
    want = ref.detach()
    if exact:
        assert torch.equal(o, want)
    else:
        assert (o - want).abs().max().item() <= OUT_TOL[3] * want.abs().max().item() + 1e-6
    assert torch.equal(y16.cpu().view(torch.int16), y.to(torch.float16).view(torch.int16))
    assert int(idx.max()) <= 8
    if exact:
        go = torch.randn(B, Cc, Po, Qo, generator=gen)
        ref.backward(go.double())
        gin = torch.full((B, H0, W0, Cc), float("nan"), device=dev)
        lib.check(lib.op_maxpool_bwd(0, K(idx), K(_nhwc(go, torch.float32, dev)), K(gin), B, H0, W0, Cc, None))
        dev_sync(dev)
        wantg = a.grad.permute(0, 2, 3, 1)
        assert (gin.cpu().double() - wantg).abs().max().item() <= OUT_TOL[0] * max(1.0, wantg.abs().max().item())
    # without idx / y16 (the inference pass): the same pooled values
    out2 = torch.full((B, Po, Qo, 2 * Cc), float("nan"), dtype=torch.float16, device=dev)
    lib.check(lib.op_bn_relu_maxpool_h2(K(y.to(dev)), K(coef), K(out2), None, None, B, H0, W0, Cc, None))
    dev_sync(dev)
    assert torch.equal(out2.cpu().view(torch.int16), oh.view(torch.int16))


def check_avgpool_h2(lib, dev, B, HW, Cc, seed=6):
    """global average pool of an h2 activation (avgpool_fwd_h2_kernel) and its two backward forms -- fp32 gradient
    (avgpool_bwd_h2_kernel, dtype 3) and fp16 gradient (avgpool_bwd_kernel<half> with gate_h2, dtype 4) -- gated by the hi halves of
    that activation, vs fp64 on the values the h2 tensor holds; outputs NaN-filled beforehand"""
    _fresh()
    gen = torch.Generator().manual_seed(seed)
    xh = to_h2(torch.relu(torch.randn(B, HW, Cc, generator=gen)))
    x_d = xh.to(dev)
    want = from_h2(xh).double().mean(1)
    out = torch.full((B, Cc), float("nan"), device=dev)
    lib.check(lib.op_avgpool_fwd_h2(K(x_d), K(out), B, HW, Cc, None))
    dev_sync(dev)
    assert (out.cpu().double() - want).abs().max().item() <= OUT_TOL[3] * want.abs().max().item() + 1e-6
    gp = torch.randn(B, Cc, generator=gen)
    full = (gp.double() / HW)[:, None, :].expand(B, HW, Cc)
    gated = torch.where(h2_hi(xh) > 0, full, torch.zeros_like(full))
    for dtype, td, tol in ((3, torch.float32, OUT_TOL[3]), (4, torch.float16, OUT_TOL[1])):
        for gate, ref in ((x_d, gated), (None, full)):
            g = torch.full((B, HW, Cc), float("nan"), dtype=td, device=dev)
            lib.check(lib.op_avgpool_bwd(dtype, K(gp.to(dev)), K(g), K(gate), B, HW, Cc, None))
            dev_sync(dev)
            err = (g.cpu().double() - ref).abs().max().item()
            assert err <= tol * ref.abs().max().item() + 1e-6, (dtype, gate is not None, err)


def check_widen_f16(lib, dev, n, seed=8):
    """widen_f16_kernel: every fp16 value (random bit patterns: subnormals, infinities, both zeros; NaNs excluded) -> the same fp32"""
    _fresh()
    gen = torch.Generator().manual_seed(seed)
    bits = torch.randint(-32768, 32768, (n,), generator=gen, dtype=torch.int32).to(torch.int16)
    h = bits.view(torch.float16)
    h = torch.where(torch.isnan(h), torch.zeros_like(h), h)
    out = torch.full((n,), float("nan"), device=dev)
    lib.check(lib.op_widen_f16(K(h.to(dev)), K(out), n, None))
    dev_sync(dev)
    assert torch.equal(out.cpu().view(torch.int32), h.float().view(torch.int32))


# ---- criteria ---------------------------------------------------------------------------------------
def golden_cases(golden_dir, name="criteria.npz"):
    z = np.load(os.path.join(golden_dir, name))
    out = {}
    for k in z.files:
        c, f = k.split("/")
        out.setdefault(c, {})[f] = z[k]
    return out


def run_criterion(lib, dev, mode, pred, targ, s4, grad_scale=1.0, want_vos=False):
    pred, targ = pred.float().contiguous().to(dev), targ.float().contiguous().to(dev)
    n = pred.shape[0]
    T = 1 if mode == 0 else (pred.shape[1] if mode == 1 else pred.shape[1] // 2)
    loss = torch.zeros(1, device=dev)
    dp = torch.zeros_like(pred)
    ds = torch.zeros(4, device=dev)
    vos = torch.zeros(n, max(T - 1, 1), 6, device=dev) if want_vos else None
    lib.check(lib.op_criterion(mode, n, T, K(pred), K(targ), K(torch.tensor(s4, dtype=torch.float32, device=dev)),
                               K(loss), K(dp), K(ds), K(vos), f32(grad_scale), None))
    dev_sync(dev)
    return loss.item(), dp.cpu(), ds.cpu(), (vos.cpu() if want_vos else None)


def check_criterion_golden(lib, dev, golden_dir):
    _fresh()
    cases = golden_cases(golden_dir)
    for name, d in cases.items():
        mode = 0 if name.startswith("posenet") else 1 if name.startswith("mapnet") else 3 if name.startswith("gps") else 2
        s4 = [float(d.get("s_" + n, 0.0)) for n in ("sax", "saq", "srx", "srq")]
        loss, dp, ds, _ = run_criterion(lib, dev, mode, torch.from_numpy(d["pred"]), torch.from_numpy(d["targ"]), s4)
        assert abs(loss - float(d["loss"])) <= 1e-5 * max(1.0, abs(float(d["loss"]))), name
        want = d["dpred"]
        if name == "online_nan":
            # same NaN pattern as the reference's autograd; finite entries agree
            assert np.array_equal(np.isnan(dp.numpy()), np.isnan(want)), name
            m = ~np.isnan(want)
            np.testing.assert_allclose(dp.numpy()[m], want[m], rtol=1e-4, atol=1e-6, err_msg=name)
            continue
        np.testing.assert_allclose(dp.numpy(), want, rtol=2e-4, atol=2e-6, err_msg=name)
        for i, n in enumerate(("sax", "saq", "srx", "srq")):
            if "d_" + n in d:
                assert abs(ds[i].item() - float(d["d_" + n])) <= 1e-4 * max(1.0, abs(float(d["d_" + n]))), (name, n)


def check_criterion_vs_oracle(lib, dev, mode_name, N, T, seed=0):
    """fused criterion kernel (loss, d pred, d s) vs the oracle criterion under fp64 autograd on seeded poses, for
    window lengths and batch sizes the golden vectors (all T = 3) do not hold"""
    _fresh()
    from oracle import criterion as OC
    gps = mode_name == "gps"
    om = {"posenet": "posenet", "mapnet": "mapnet", "online": "mapnet++", "gps": "mapnet++"}[mode_name]
    _, targ = oracle.make_batch(om, N, 1, 1, t=T, seed=100 + seed, gps_mode=gps)
    gen = torch.Generator().manual_seed(seed)
    shape = (N, 6) if mode_name == "posenet" else (N, T, 6) if mode_name == "mapnet" else (N, 2 * T, 6)
    lead = targ if mode_name in ("posenet", "mapnet") else torch.cat((targ[:, :T], oracle.make_batch("mapnet", N, 1, 1, t=T, seed=7 + seed)[1]), 1)
    pred = (lead + 0.3 * torch.randn(*shape, generator=gen)).contiguous()
    s4 = [0.3, -2.5, 0.7, -3.5]
    kw = dict(sax=s4[0], saq=s4[1], learn_beta=True)
    if mode_name == "posenet":
        crit, mode = OC.PoseNetCriterion(**kw), 0
    elif mode_name == "mapnet":
        crit, mode = OC.MapNetCriterion(srx=s4[2], srq=s4[3], learn_gamma=True, **kw), 1
    else:
        crit, mode = OC.MapNetOnlineCriterion(srx=s4[2], srq=s4[3], learn_gamma=True, gps_mode=gps, **kw), (3 if gps else 2)
    crit = crit.double()
    p64 = pred.double().requires_grad_(True)
    want = crit(p64, targ.double())
    want.backward()
    loss, dp, ds, _ = run_criterion(lib, dev, mode, pred, targ, s4)
    assert abs(loss - want.item()) <= 2e-5 * max(1.0, abs(want.item())), (mode_name, N, T)
    np.testing.assert_allclose(dp.numpy(), p64.grad.float().numpy(), rtol=3e-4, atol=3e-6, err_msg=str((mode_name, N, T)))
    names = ("sax", "saq") if mode_name == "posenet" else ("sax", "saq", "srx") if gps else ("sax", "saq", "srx", "srq")
    for i, n in enumerate(names):
        w = getattr(crit, n).grad.item()
        assert abs(ds[i].item() - w) <= 2e-4 * max(1.0, abs(w)), (mode_name, N, T, n)


def check_calc_vos_golden(lib, dev, golden_dir):
    _fresh()
    z = np.load(os.path.join(golden_dir, "pose_algebra.npz"))
    poses = torch.from_numpy(z["poses"]).float().to(dev)
    cot = torch.from_numpy(z["cot"]).float().to(dev)
    N, T = poses.shape[0], poses.shape[1]
    vos = torch.zeros(N, T - 1, 6, device=dev)
    dpo = torch.zeros_like(poses)
    lib.check(lib.op_calc_vos(K(poses), N, T, K(vos), K(cot), K(dpo), None))
    dev_sync(dev)
    np.testing.assert_allclose(vos.cpu().numpy(), z["calc_vos"], atol=2e-6)
    np.testing.assert_allclose(dpo.cpu().numpy(), z["calc_vos_vjp"], rtol=1e-4, atol=2e-5)
    # identity: the relative pose of a pose w.r.t. itself is zero (pose_utils.calc_vo_logq(p, p))
    same = poses[:, :1].repeat(1, 2, 1).contiguous()
    v2 = torch.zeros(N, 1, 6, device=dev)
    lib.check(lib.op_calc_vos(K(same), N, 2, K(v2), None, None, None))
    dev_sync(dev)
    assert float(v2.abs().max()) < 1e-6


def check_adam(lib, dev, n=10007, steps=3, max_norm=0.0, wd=5e-4, seed=6):
    _fresh()
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1e-3, weight_decay=wd)
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    for step in range(1, steps + 1):
        g = torch.randn(n, generator=gen) * (5.0 if step == 1 else 0.1)
        pt.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        lib.check(lib.op_adam(K(p), K(g.to(dev)), K(m), K(v), n, n, f32(1e-3), f32(wd), f32(0.9), f32(0.999), f32(1e-8),
                              step, f32(1.0), f32(max_norm), K(sq), 0, None))
        dev_sync(dev)
        # Adam's update m/(sqrt(v)+eps) is ill-conditioned where |g| ~ eps: allow a 1e-5 fraction of
        # elements to differ by (much) less than one step, everything else must agree tightly
        d = (p.cpu() - pt.detach()).abs()
        bad = d > (2e-6 + 1e-5 * pt.detach().abs())
        assert bad.float().mean().item() <= 1e-5 and d.max().item() <= 2e-3


def check_sgd_rmsprop(lib, dev, method, n=10007, steps=4, max_norm=0.0, wd=5e-4, seed=6, **kw):
    """the fused update in its SGD / RMSprop forms (common/optimizer.py:16-26) vs torch.optim.SGD / RMSprop"""
    _fresh()
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    pt = p0.clone().requires_grad_(True)
    if method == "sgd":
        opt = torch.optim.SGD([pt], lr=1e-2, weight_decay=wd, **kw)
        mid, nest = 1, int(kw.get("nesterov", False))
        b1, b2, eps = kw.get("momentum", 0.0), kw.get("dampening", 0.0), 0.0
    else:
        opt = torch.optim.RMSprop([pt], lr=1e-3, weight_decay=wd, **kw)
        mid, nest = 2, 0
        b1, b2, eps = kw.get("momentum", 0.0), kw.get("alpha", 0.99), kw.get("eps", 1e-8)
    lr = opt.param_groups[0]["lr"]
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    for step in range(1, steps + 1):
        g = torch.randn(n, generator=gen) * (5.0 if step == 1 else 0.1)
        pt.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        lib.check(lib.op_optim(mid, nest, K(p), K(g.to(dev)), K(m), K(v), n, n, f32(lr), f32(wd), f32(b1), f32(b2), f32(eps),
                               step, f32(1.0), f32(max_norm), K(sq), 0, None))
        dev_sync(dev)
        # g / (sqrt(square_avg) + eps) is ill-conditioned where the clipped gradient and weight_decay * p nearly cancel
        # (|g| ~ 1e-6: about 1e-4 of the elements); those may differ by a fraction of one step, the rest must agree tightly
        d = (p.cpu() - pt.detach()).abs()
        bad = d > (2e-6 + 1e-5 * pt.detach().abs())
        frac = 1e-5 if method == "sgd" else 1e-3
        assert bad.float().mean().item() <= frac and d.max().item() <= 2e-3, (step, bad.float().mean().item(), d.max().item())
    st = opt.state[pt]
    for key, mine in (("momentum_buffer", m), ("square_avg", v)):
        if key in st:  # the same ill-conditioned elements carry their difference into RMSprop's momentum buffer
            dd = (mine.cpu() - st[key]).abs()
            badm = dd > 1e-5 * max(1.0, st[key].abs().max().item())
            assert badm.float().mean().item() <= (0.0 if method == "sgd" else 1e-3), (key, badm.float().mean().item())


def check_train_other_optimizers(lib, dev, method, N=1, H=32, W=40, steps=2, **kw):
    """step_feedfwd with Optimizer(method='sgd' | 'rmsprop') vs the oracle's torch.optim counterpart: parameters after
    `steps` steps, the optimiser state in torch's state_dict format, the SGD step schedule of the wrapper"""
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype("fp32")
    onet, net = build_pair(lib, dev)
    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    oc = oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True)
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    og = [{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}]
    gg = [{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}]
    lr = 1e-4 if method == "sgd" else 1e-5
    oopt = oracle.Optimizer(og, method, base_lr=lr, weight_decay=5e-4, **dict(kw))
    opt = G.Optimizer(gg, method, base_lr=lr, weight_decay=5e-4, **dict(kw))
    if method == "sgd":  # the wrapper's step schedule (common/optimizer.py:28-42)
        for ep in (0, 3, 7):
            assert abs(opt.adjust_lr(ep) - oopt.adjust_lr(ep)) < 1e-12
            assert opt.learner.param_groups[0]["lr"] == oopt.learner.param_groups[0]["lr"]
        opt.adjust_lr(0), oopt.adjust_lr(0)
    onet.train()
    net.train()
    p_init = {k: v.detach().clone() for k, v in onet.named_parameters()}

    def displacement():
        dev_sync(dev)
        hp = dict(net.named_parameters())
        num = den = 0.0
        for k, v in onet.named_parameters():
            d_or = (v.detach() - p_init[k]).double()
            d_hip = (hp[k].detach().cpu() - p_init[k]).double()
            num += float((d_hip - d_or).pow(2).sum())
            den += float(d_or.pow(2).sum())
        assert den > 0
        return (num / den) ** 0.5

    rel = []
    for step in range(steps):
        lo, po = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True, 0.0)
        l, p = G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True, 0.0)
        if step == 0:
            assert abs(l - lo) <= 1e-4 * max(1.0, abs(lo)), (l, lo)
        rel.append(displacement())
    # the first step's update is the optimiser formula applied to gradients that agree to ~1e-3; later steps also carry
    # the network's own amplification of that difference (tools/oracle_sensitivity.py) and the momentum / square-average
    # state of the first
    # (RMSprop's first update g / sqrt((1 - alpha) g^2) is sign-like: every element whose tiny gradient changes sign moves
    # the other way by a full step -- see the ReLU-gate note in DESIGN.md section 6)
    assert rel[0] < (2e-2 if method == "sgd" else 0.15) and rel[-1] < 0.3, rel
    # state in torch's format: loadable by the real optimiser, same keys as the oracle's
    sd, osd = opt.learner.state_dict(), oopt.learner.state_dict()
    assert set(sd["state"].keys()) == set(osd["state"].keys())
    for k in osd["state"]:
        assert set(sd["state"][k].keys()) == set(osd["state"][k].keys()), (sd["state"][k].keys(), osd["state"][k].keys())
    oopt.learner.load_state_dict(sd)
    return rel


# ---- whole network --------------------------------------------------------------------------------------
def build_pair(lib, dev, seed=7, filter_nans=False):
    import geomapnet_amd as G
    torch.manual_seed(seed)
    onet = oracle.MapNet(oracle.PoseNet(oracle.resnet34(), droprate=0.0, pretrained=False, filter_nans=filter_nans))
    net = G.MapNet(G.PoseNet(G.resnet34(_binding=lib), droprate=0.0, pretrained=False, filter_nans=filter_nans, _binding=lib))
    net.load_state_dict(onet.state_dict())
    if torch.device(dev).type == "cuda":
        net.cuda()
    return onet, net


def grad_views(net):
    eng = net.mapnet._engine
    return {e.name.decode(): _view(eng.grads(), e) for e in eng.entries if not e.is_buffer}


def _record_deviation(rec):
    """MN_RECORD_DEVIATIONS=<file>: every oracle-differential step appends what it measured (tools/fp16_envelope: the fp16 gates of the
    suite are set at 1.5x these numbers)"""
    path = os.environ.get("MN_RECORD_DEVIATIONS")
    if path:
        import json
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def check_train_step(lib, dev, dtype_name, mode="mapnet", N=2, H=64, W=85, steps=1, max_grad_norm=0.0, lr=1e-4, wd=5e-4,
                     loss_rtol=1e-4, pose_atol=1e-3, grad_l2_rtol=2e-2, gps=False, filter_nans=False, adam_eps=None,
                     pose_abs=None, later_tol=None, crit_grad_rtol=1e-3):
    """one (or more) full training steps, HIP library vs the oracle on identical inputs and weights.
    adam_eps: Adam's epsilon for both sides.  With the default 1e-8 the update m/(sqrt(v)+eps) is +-1 for every element
    however small its gradient, so last-bit differences of near-zero gradients move parameters by a full lr and later
    steps can only be compared loosely; with an epsilon above the gradient noise the update is smooth in the gradient
    and EVERY step is held to (loss_rtol, pose_atol) -- that pins the multi-step state (moments, step count, running
    statistics, weight repacking) at the first step's tolerance."""
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    onet, net = build_pair(lib, dev, filter_nans=filter_nans)
    x, t = oracle.make_batch(mode, N, H, W, seed=7, gps_mode=gps)
    if mode == "posenet":
        onet, net = onet.mapnet, net.mapnet
        oc = oracle.PoseNetCriterion(0.0, -3.0, True)
        c = G.PoseNetCriterion(sax=0.0, saq=-3.0, learn_beta=True, _binding=lib)
        og = [{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}]
        gg = [{"params": net.parameters()}, {"params": [c.sax, c.saq]}]
    else:
        if mode == "mapnet":
            oc = oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True)
            c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
        else:
            oc = oracle.MapNetOnlineCriterion(0.0, -3.0, 0.0, -3.0, True, True, gps_mode=gps)
            c = G.MapNetOnlineCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, gps_mode=gps,
                                        _binding=lib)
        og = [{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}]
        gg = [{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}]
    kw = {} if adam_eps is None else {"eps": adam_eps}
    p_init = {k: v.detach().clone() for k, v in onet.named_parameters()}
    oopt = oracle.Optimizer(og, "adam", base_lr=lr, weight_decay=wd, **kw)
    opt = G.Optimizer(gg, "adam", base_lr=lr, weight_decay=wd, **kw)
    onet.train()
    net.train()
    report = []
    for step in range(steps):
        lo, po = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True, max_grad_norm)
        l, p = G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True, max_grad_norm)
        pose_err = (p.cpu() - po.detach()).abs().max().item()
        report.append((l, lo, pose_err))
        _record_deviation({"dtype": dtype_name, "mode": mode, "N": N, "H": H, "W": W, "step": step, "gps": bool(gps),
                           "loss_rel": abs(l - lo) / max(1.0, abs(lo)), "pose_abs_max": pose_err, "dev": str(dev)})
        # steps after the first start from Adam's sign-like first update (m/sqrt(v) = +-1 for every element,
        # however small its gradient), which amplifies summation-order noise: compared loosely
        # (later_tol: (loss, pose) for the steps after the first when a mode's measured second-step deviation is known -- fp16)
        lt, pt = (loss_rtol, pose_atol) if step == 0 or adam_eps is not None else (
            later_tol if later_tol is not None else (max(loss_rtol, 5e-3), max(pose_atol, 2e-2)))
        assert abs(l - lo) <= lt * max(1.0, abs(lo)), (step, l, lo)
        assert pose_err <= pt * max(1.0, po.abs().max().item()), (step, pose_err)
        # the north-star bar as written -- max abs over all predicted components, not relative to the pose scale -- for the first
        # step of every fp32-class mode whatever the shape, and wherever a caller asks for it
        if pose_abs is None and dtype_name in ("fp32", "fp32x3", "fp16x2", "fp16x2m") and pose_atol <= 2e-3:
            pose_abs = 1e-3
        if step == 0 and pose_abs is not None:
            assert pose_err <= pose_abs, (step, pose_err)
        if step == 0 and (grad_l2_rtol is not None or os.environ.get("MN_RECORD_DEVIATIONS")) and max_grad_norm == 0.0:
            eng = (net.mapnet if hasattr(net, "mapnet") else net)._engine
            prefix = "mapnet." if hasattr(onet, "mapnet") else ""
            og_ = dict(onet.named_parameters())
            worst = 0.0
            for e in eng.entries:
                if e.is_buffer:
                    continue
                name = e.name.decode()
                g = _view(eng.grads(), e).cpu().double()
                r = og_[prefix + name].grad.double()
                if r.norm() < 1e-8:
                    continue
                worst = max(worst, ((g - r).norm() / r.norm()).item())
            _record_deviation({"dtype": dtype_name, "mode": mode, "N": N, "H": H, "W": W, "grad_worst_tensor": worst, "dev": str(dev)})
            if grad_l2_rtol is None:
                continue
            assert worst <= grad_l2_rtol, worst
            cg = eng.grads()[-4:].cpu().numpy()
            names = ("sax", "saq", "srx", "srq")
            for i, nm in enumerate(names):
                if hasattr(oc, nm) and getattr(oc, nm).grad is not None:
                    # d loss / d s = 1 - e^-s * (its mean term): e^-s = 20 at s = -3 amplifies the mean term's deviation (fp16 measures
                    # 4.0e-3 / 2.3e-3 relative at the suite's two shapes: FP16_SMALL)
                    ref = getattr(oc, nm).grad.item()
                    _record_deviation({"dtype": dtype_name, "mode": mode, "N": N, "H": H, "W": W, "crit_grad": nm,
                                       "rel": abs(cg[i] - ref) / max(1.0, abs(ref)), "dev": str(dev)})
                    assert abs(cg[i] - ref) <= crit_grad_rtol * max(1.0, abs(ref)), (nm, cg[i], ref)
    if adam_eps is not None:
        # total displacement of the parameters over all steps: the optimiser-state dynamics (moments carried from step to
        # step, bias corrections, weight decay) seen directly, not through the next loss
        dev_sync(dev)
        hp = dict(net.named_parameters())
        num = den = 0.0
        for k, v in onet.named_parameters():
            d_or = (v.detach() - p_init[k]).double()
            d_hip = (hp[k].detach().cpu() - p_init[k]).double()
            num += float((d_hip - d_or).pow(2).sum())
            den += float(d_or.pow(2).sum())
        report.append(("displacement_rel_l2", (num / den) ** 0.5))
    return report


def check_dropout(lib, dev, dtype_name="fp32", N=2, H=64, W=85, p_drop=0.5, seed=1234, loss_rtol=1e-4, pose_atol=1e-3,
                  grad_l2_rtol=2e-2, wiring=True):
    """F.dropout(x, p) between the feature ReLU and the pose heads (models/posenet.py:68-69) on the device: one MapNet training
    step with PoseNet(droprate=0.5, dropout_active=True) against the oracle applying THE SAME mask (read back from the device);
    the mask itself (values, keep rate, a fresh draw per step, reproducible from the seed); eval() does not drop"""
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    torch.manual_seed(7)
    onet = oracle.MapNet(oracle.PoseNet(oracle.resnet34(), droprate=p_drop, pretrained=False))
    sd0 = {k: v.clone() for k, v in onet.state_dict().items()}

    def hip_net():
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # dropout_active=True must not trigger the identity warning
            net = G.MapNet(G.PoseNet(G.resnet34(_binding=lib), droprate=p_drop, pretrained=False, dropout_active=True,
                                     dropout_seed=seed, _binding=lib))
        net.load_state_dict(sd0)
        if torch.device(dev).type == "cuda":
            net.cuda()
        return net

    net = hip_net()
    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    oc = oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True)
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    oopt = oracle.Optimizer([{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}], "adam",
                            base_lr=1e-4, weight_decay=5e-4)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    onet.train()
    net.train()
    l, p = G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True, 0.0)
    eng = net.mapnet._engine
    plan = next(iter(eng.plans.values()))
    mask = eng.dropout_mask(plan).cpu()
    keep = 1.0 / (1.0 - p_drop)
    assert mask.shape == (N * 3, 2048)
    assert bool(((mask == 0) | ((mask - keep).abs() < 1e-6)).all()), "mask values must be 0 or 1/(1-p)"
    frac = (mask == 0).float().mean().item()
    assert abs(frac - p_drop) < 5.0 * (p_drop * (1 - p_drop) / mask.numel()) ** 0.5 + 1e-3, frac
    # the oracle with the device's mask
    onet.mapnet.dropout_mask = mask
    lo, po = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True, 0.0)
    assert abs(l - lo) <= loss_rtol * max(1.0, abs(lo)), (l, lo)
    assert (p.cpu() - po.detach()).abs().max().item() <= pose_atol, (p.cpu() - po.detach()).abs().max().item()
    og_ = dict(onet.named_parameters())
    worst = 0.0
    for e in eng.entries:
        if e.is_buffer:
            continue
        g = _view(eng.grads(), e).cpu().double()
        r = og_["mapnet." + e.name.decode()].grad.double()
        if r.norm() > 1e-8:
            worst = max(worst, ((g - r).norm() / r.norm()).item())
    assert worst <= grad_l2_rtol, worst
    res = {"loss": l, "loss_oracle": lo, "dropped_fraction": frac, "grad_worst": worst}
    if not wiring:  # (the emulator suite stops here: what follows re-runs the step to test host-side wiring)
        return res
    # a second training step draws a different mask; a model built from the same seed draws the same first mask
    G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True, 0.0)
    mask2 = eng.dropout_mask(plan).cpu()
    assert not torch.equal(mask, mask2)
    net_b = hip_net()
    net_b.train()
    cb = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    optb = G.Optimizer([{"params": net_b.parameters()}, {"params": [cb.sax, cb.saq]}, {"params": [cb.srx, cb.srq]}], "adam",
                       base_lr=1e-4, weight_decay=5e-4)
    G.step_feedfwd(x.to(dev), net_b, dev != "cpu", t.to(dev), cb, optb, True, 0.0)
    eb = net_b.mapnet._engine
    assert torch.equal(eb.dropout_mask(next(iter(eb.plans.values()))).cpu(), mask)
    # eval(): no dropout (nn.Dropout semantics) -- the forward pass equals the oracle's without a mask
    onet2 = oracle.MapNet(oracle.PoseNet(oracle.resnet34(), droprate=p_drop, pretrained=False))
    onet2.load_state_dict(sd0)
    onet2.eval()
    net_c = hip_net()
    net_c.eval()
    with torch.no_grad():
        ref = onet2(x)
    out = net_c(x.to(dev))
    assert (out.cpu() - ref).abs().max().item() <= pose_atol * max(1.0, ref.abs().max().item())
    return res


def check_eval_forward(lib, dev, dtype_name, B=3, H=64, W=85, atol=1e-3):
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    onet, net = build_pair(lib, dev)
    onet, net = onet.mapnet, net.mapnet
    x, _ = oracle.make_batch("posenet", B, H, W, seed=11)
    onet.eval()
    net.eval()
    with torch.no_grad():
        ref = onet(x)
    out = net(x.to(dev))
    err = (out.cpu() - ref).abs().max().item()
    _record_deviation({"check": "eval_forward", "dtype": dtype_name, "B": B, "H": H, "W": W, "pose_abs_max": err,
                       "scale": ref.abs().max().item(), "dev": str(dev)})
    assert err <= atol * max(1.0, ref.abs().max().item())


def check_eval_flow(lib, dev, dtype_name, L=4, T=3, H=64, W=85, rtol=2e-3, check_q=True):
    """scripts/eval.py flow (window in, middle prediction kept, qexp, un-normalise, median/mean errors):
    geomapnet_amd.evaluate on the HIP forward vs the oracle forward + the oracle's numpy metric"""
    _fresh()
    import numpy as np
    import geomapnet_amd as G
    from geomapnet_amd import evaluate as E
    from oracle import pose_math
    G.set_compute_dtype(dtype_name)
    onet, net = build_pair(lib, dev)
    x, t = oracle.make_batch("mapnet", L, H, W, seed=21)
    pose_m, pose_s = np.array([0.5, -1.0, 2.0]), np.array([2.0, 3.0, 0.5])
    batches = [(x[i:i + 1].to(dev), t[i:i + 1]) for i in range(L)]
    summary, pred7, targ7 = E.evaluate(net, batches, pose_m, pose_s, cuda=(dev != "cpu"))
    assert pred7.shape == (L, 7) and targ7.shape == (L, 7)
    onet.eval()
    want_t, want_q = [], []
    with torch.no_grad():
        for i in range(L):
            o = onet(x[i:i + 1]).numpy().reshape(-1, 6)
            g = t[i:i + 1].numpy().reshape(-1, 6)
            mid = len(o) // 2
            po = np.hstack((o[mid, :3] * pose_s + pose_m, pose_math.qexp_np(o[mid, 3:])))
            pg = np.hstack((g[mid, :3] * pose_s + pose_m, pose_math.qexp_np(g[mid, 3:])))
            want_t.append(np.linalg.norm(po[:3] - pg[:3]))
            want_q.append(pose_math.quaternion_angular_error(po[3:], pg[3:]))
    want = [np.median(want_t), np.mean(want_t), np.median(want_q), np.mean(want_q)]
    got = [summary["median_t"], summary["mean_t"], summary["median_q"], summary["mean_q"]]
    # check_q=False: with random-init weights and eval-mode BatchNorm the predicted log-quaternions are hundreds
    # of radians, so the wrapped rotation error is chaotic in the last bits of the pose (fp16 runs)
    k = 4 if check_q else 2
    _record_deviation({"check": "eval_flow", "dtype": dtype_name, "L": L, "H": H, "W": W, "dev": str(dev),
                       "max_abs_diff": float(np.max(np.abs(np.asarray(got[:k]) - np.asarray(want[:k])))),
                       "max_rel_diff": float(np.max(np.abs(np.asarray(got[:k]) - np.asarray(want[:k])) / (np.abs(np.asarray(want[:k])) + 1e-12)))})
    np.testing.assert_allclose(got[:k], want[:k], rtol=rtol, atol=rtol)
    return summary


def check_checkpoint_interop(lib, dev, H=40, W=53, resume_step=True):
    """optimiser / criterion / model state in the reference's checkpoint format: torch.optim.Adam-shaped
    state_dict (loadable by a real torch Adam over the oracle's parameters, moments equal to the oracle's),
    save -> load -> resume reproduces the next step, prefix logic of common/train.py:22-53"""
    _fresh()
    import numpy as np
    import geomapnet_amd as G
    G.set_compute_dtype("fp32")

    def make(seed=7):
        onet, net = build_pair(lib, dev, seed=seed)
        oc = oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True)
        c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
        og = [{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}]
        gg = [{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}]
        return (onet, oc, oracle.Optimizer(og, "adam", base_lr=1e-4, weight_decay=5e-4),
                net, c, G.Optimizer(gg, "adam", base_lr=1e-4, weight_decay=5e-4))

    onet, oc, oopt, net, c, opt = make()
    assert opt.learner.state_dict()["state"] == {}  # as torch before the first step
    x, t = oracle.make_batch("mapnet", 1, H, W, seed=7)
    onet.train()
    net.train()
    oracle.step_feedfwd(x, onet, False, t, oc, oopt, True)
    G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True)
    sd = opt.learner.state_dict()
    osd = oopt.learner.state_dict()
    assert set(sd.keys()) == {"state", "param_groups"}
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in osd["param_groups"]]
    assert sorted(sd["state"].keys()) == sorted(osd["state"].keys())
    num = den = 0.0
    for k, st in sd["state"].items():
        assert int(st["step"]) == 1 and tuple(st["exp_avg"].shape) == tuple(osd["state"][k]["exp_avg"].shape)
        assert st["exp_avg"].is_contiguous()
        num += (st["exp_avg"].cpu().double() - osd["state"][k]["exp_avg"].double()).pow(2).sum().item()
        den += osd["state"][k]["exp_avg"].double().pow(2).sum().item()
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5
    # a real torch.optim.Adam accepts it
    probe = torch.optim.Adam([{"params": list(onet.parameters())}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}],
                             lr=1e-4, weight_decay=5e-4)
    probe.load_state_dict({"state": {k: {a: (b.cpu() if torch.is_tensor(b) else b) for a, b in v.items()} for k, v in sd["state"].items()},
                           "param_groups": sd["param_groups"]})
    # and the oracle's (genuine torch) state loads into the fused optimiser bit-exactly
    onet2, oc2, oopt2, net2, c2, opt2 = make(seed=8)
    opt2.learner.load_state_dict(osd)
    ckpt = G.save_checkpoint(None, 3, net, opt, c)
    import io
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    buf.seek(0)
    ckpt = torch.load(buf, map_location="cpu", weights_only=False)
    assert G.load_checkpoint(ckpt, net2, opt2, c2, resume_optim=True) == 3
    net2.train()
    if not resume_step:  # (emulator runs) state equality after the load instead of one more step on both replicas
        from geomapnet_amd.train import _bind
        _bind(net2.mapnet._engine, c2, opt2)
        sd2 = opt2.learner.state_dict()
        for k, st in sd["state"].items():
            assert int(sd2["state"][k]["step"]) == 1
            assert torch.equal(sd2["state"][k]["exp_avg"].cpu(), st["exp_avg"].cpu())
            assert torch.equal(sd2["state"][k]["exp_avg_sq"].cpu(), st["exp_avg_sq"].cpu())
        for (k1, v1), (k2, v2) in zip(net.state_dict().items(), net2.state_dict().items()):
            assert k1 == k2 and torch.equal(v1.cpu(), v2.cpu()), k1
        for k in ("sax", "saq", "srx", "srq"):
            assert float(getattr(c, k).detach()) == float(getattr(c2, k).detach())
        G.load_state_dict(net2, net.mapnet.state_dict())
        G.load_state_dict(net2.mapnet, net.state_dict())
        return
    l1, p1 = G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True)
    l2, p2 = G.step_feedfwd(x.to(dev), net2, dev != "cpu", t.to(dev), c2, opt2, True)
    assert abs(l1 - l2) <= 1e-5 * max(1.0, abs(l1)), (l1, l2)
    assert (p1 - p2).abs().max().item() <= 1e-5
    sd1, sd2 = opt.learner.state_dict(), opt2.learner.state_dict()
    assert int(sd2["state"][0]["step"]) == 2
    worst = max((sd1["state"][k]["exp_avg_sq"] - sd2["state"][k]["exp_avg_sq"]).abs().max().item() /
                (sd1["state"][k]["exp_avg_sq"].abs().max().item() + 1e-30) for k in sd1["state"])
    assert worst < 1e-3, worst
    for k in ("sax", "saq", "srx", "srq"):
        assert abs(float(getattr(c, k).detach()) - float(getattr(c2, k).detach())) < 1e-6
    # prefix logic: PoseNet-named state into MapNet and back (common/train.py:22-53)
    G.load_state_dict(net2, net.mapnet.state_dict())
    G.load_state_dict(net2.mapnet, net.state_dict())
    try:
        G.load_state_dict(net2, {"unrelated.weight": torch.zeros(1)})
        raise AssertionError("expected KeyError")
    except KeyError:
        pass


def check_u8_input(lib, dev, N=1, H=40, W=53, dtype_name="fp32"):
    """device-side ToTensor + Normalize: uint8 NHWC input vs the same images normalised on the host (fp32 NCHW),
    forward and one training step against the oracle (fp16x2m: the stem's backward kernels read a second, fp16 image of the input
    produced by the same conversion -- the stem's weight gradient is compared as well)"""
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    onet, net = build_pair(lib, dev)
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (N, 3, H, W, 3), generator=g, dtype=torch.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    x = ((u8.float() / 255.0 - torch.tensor(mean)) / torch.tensor(std)).permute(0, 1, 4, 2, 3).contiguous()
    _, t = oracle.make_batch("mapnet", N, 8, 8, seed=7)
    net.eval()
    onet.eval()
    with torch.no_grad():
        ref = onet(x)
    net.set_input_u8(mean, std)
    got = net(u8.to(dev)).cpu()
    assert (got - ref).abs().max().item() <= 1e-3 * max(1.0, ref.abs().max().item())
    try:
        net(x.to(dev))
        raise AssertionError("fp32 input must be rejected in uint8 mode")
    except (ValueError, G._binding.MapNetHipError):
        pass
    oc = oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True)
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    oopt = oracle.Optimizer([{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}], "adam",
                            base_lr=1e-4, weight_decay=5e-4)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    onet.train()
    net.train()
    lo, po = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True)
    l, p = G.step_feedfwd(u8.to(dev), net, dev != "cpu", t.to(dev), c, opt, True)
    assert abs(l - lo) <= 1e-4 * max(1.0, abs(lo)), (l, lo)
    assert (p.cpu() - po.detach()).abs().max().item() <= 2e-3 * max(1.0, po.abs().max().item())
    gw = grad_views(net)["feature_extractor.conv1.weight"].cpu().double()
    rw = dict(onet.named_parameters())["mapnet.feature_extractor.conv1.weight"].grad.double()
    assert ((gw - rw).norm() / rw.norm()).item() <= 2e-2, ((gw - rw).norm() / rw.norm()).item()
    net.set_input_u8(None)
    assert net.mapnet._engine.input_u8 is None


# ---- pose-graph optimisation (csrc/pgo.h vs oracle/pgo.py and the golden vectors of the reference) -------------
PGO_TOL = 1e-9  # fp64 on both sides; the only differences are summation order and libm vs device sin/cos/sqrt


def check_pgo_golden(lib, dev, golden_dir):
    """every case of tests/golden/pgo.npz (outputs of the reference's PoseGraph / PoseGraphFC, incl. its own fixture
    pgo_test_poses1): batched launch per case, one-window wrappers, optimize_poses with VOs from target poses"""
    from geomapnet_amd import pgo as P
    g = np.load(os.path.join(golden_dir, "pgo.npz"))
    for tag in g["cases"]:
        cfg = g[tag + "/cfg"]
        N, fc, sig = int(cfg[0]), bool(cfg[1]), cfg[2:]
        got = P.optimize_windows(g[tag + "/pred"], g[tag + "/vos"], fc_vos=fc, sax=sig[0], saq=sig[1], srx=sig[2], srq=sig[3],
                                 device=dev, binding=lib)
        err = np.abs(got - g[tag + "/opt"]).max()
        assert err <= PGO_TOL, (tag, err)
        # the optimisation does something: the result differs from its initialisation
        assert np.abs(got - g[tag + "/pred"]).max() > 1e-3
        # one-window class interface (reference signatures)
        cls = P.PoseGraphFC if fc else P.PoseGraph
        one = cls(device=dev, binding=lib).optimize(g[tag + "/pred"][0], g[tag + "/vos"][0], sax=sig[0], saq=sig[1], srx=sig[2],
                                                    srq=sig[3])
        assert np.abs(one - g[tag + "/opt"][0]).max() <= PGO_TOL
    # the reference's own fixture: chain graph handed the 3 fully connected VOs, reads the first two
    fx = P.optimize_poses(g["fixture/poses"], vos=g["fixture/vos"], device=dev, binding=lib)
    assert np.abs(fx - g["fixture/opt"]).max() <= PGO_TOL
    ft = P.optimize_poses(g["from_targets/pred"], target_poses=g["from_targets/targ"], srx=0.5, srq=0.5, device=dev, binding=lib)
    assert np.abs(ft - g["from_targets/opt"]).max() <= PGO_TOL
    assert P.optimize_poses(g["fixture/poses"], device=dev, binding=lib) is None  # neither VOs nor targets (:798-800)


def pgo_windows(W, N, fc, seed, noise=0.05):
    """seeded windows: smooth trajectory, exact VOs, noisy predictions (numpy only)"""
    rng = np.random.default_rng(seed)

    def qmul(a, b):
        w1, x1, y1, z1 = np.moveaxis(a, -1, 0)
        w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
        return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2, w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2], axis=-1)

    def small(shape, s):
        d = np.concatenate([np.ones(shape + (1,)), rng.normal(size=shape + (3,)) * s], axis=-1)
        return d / np.linalg.norm(d, axis=-1, keepdims=True)

    t = np.cumsum(rng.normal(size=(W, N, 3)) * 0.3, axis=1)
    q = np.zeros((W, N, 4))
    q0 = rng.normal(size=(W, 4))
    q[:, 0] = q0 / np.linalg.norm(q0, axis=-1, keepdims=True)
    for i in range(1, N):
        q[:, i] = qmul(q[:, i - 1], small((W,), 0.1))
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)] if fc else [(i, i + 1) for i in range(N - 1)]
    vos = np.zeros((W, len(pairs), 7))
    conj = np.array([1.0, -1, -1, -1])
    for k, (i, j) in enumerate(pairs):
        qi = q[:, i] * conj
        v = np.concatenate([np.zeros((W, 1)), t[:, j] - t[:, i]], axis=-1)
        vos[:, k, :3] = qmul(qi, qmul(v, q[:, i]))[:, 1:]
        vos[:, k, 3:] = qmul(qi, q[:, j])
    gt = np.concatenate([t, q], axis=-1)
    pred = gt.copy()
    pred[..., :3] += rng.normal(size=(W, N, 3)) * noise
    pred[..., 3:] = qmul(pred[..., 3:], small((W, N), noise))
    return pred, vos, gt


def check_pgo_vs_oracle(lib, dev, W=5, N=7, fc=False, seed=11, sig=(1.0, 1.0, 1.0, 1.0)):
    from geomapnet_amd import pgo as P
    from oracle import pgo as opgo
    pred, vos, _ = pgo_windows(W, N, fc, seed)
    got = P.optimize_windows(pred, vos, fc_vos=fc, sax=sig[0], saq=sig[1], srx=sig[2], srq=sig[3], device=dev, binding=lib)
    for w in range(W):
        want = opgo.optimize_window(pred[w], vos[w], fc=fc, sax=sig[0], saq=sig[1], srx=sig[2], srq=sig[3])
        assert np.abs(got[w] - want).max() <= PGO_TOL, (w, np.abs(got[w] - want).max())


def check_pgo_properties(lib, dev, W=4096, N=7, fc=True, seed=3):
    """size-independent properties at evaluation-set scale: (1) exact poses with their exact VOs are a fixed point
    (all residuals vanish, so every step is zero); (2) windows are independent: a window's result does not depend on
    the batch it is launched in; (3) error handling: a non-finite window is reported, the others are unaffected"""
    from geomapnet_amd import pgo as P
    pred, vos, gt = pgo_windows(W, N, fc, seed)
    fixed = P.optimize_windows(gt, vos, fc_vos=fc, device=dev, binding=lib)
    assert np.abs(fixed - gt).max() <= 1e-12
    full = P.optimize_windows(pred, vos, fc_vos=fc, srx=0.5, srq=0.5, device=dev, binding=lib)
    sel = np.array([0, 1, W // 2, W - 1])
    part = P.optimize_windows(pred[sel], vos[sel], fc_vos=fc, srx=0.5, srq=0.5, device=dev, binding=lib)
    assert np.array_equal(full[sel], part)
    assert np.isfinite(full).all()
    # with exact VOs and a strong relative term the optimised trajectory is closer to the truth than the prediction
    e0 = np.linalg.norm(pred[..., :3] - gt[..., :3], axis=-1).mean()
    e1 = np.linalg.norm(full[..., :3] - gt[..., :3], axis=-1).mean()
    assert e1 < e0, (e0, e1)
    bad = pred[:3].copy()
    bad[1, 2, 3:] = np.nan
    try:
        P.optimize_windows(bad, vos[:3], fc_vos=fc, device=dev, binding=lib)
        raise AssertionError("a NaN window must raise LinAlgError")
    except np.linalg.LinAlgError as e:
        assert "[1]" in str(e)
    for n_bad in (1, 13):
        try:
            P.optimize_windows(np.ones((1, n_bad, 7)), np.ones((1, n_bad * (n_bad - 1) // 2, 7)), fc_vos=True, device=dev,
                               binding=lib)
            raise AssertionError("window length out of range must be rejected")
        except lib_error():
            pass
    try:
        P.optimize_windows(pred[:2], vos[:2, :3], fc_vos=fc, device=dev, binding=lib)
        raise AssertionError("too few VOs must be rejected")
    except ValueError:
        pass


def lib_error():
    from geomapnet_amd._binding import MapNetHipError
    return MapNetHipError


# ---- NaN filter (models/posenet.py:28-34,50-51) with a REAL NaN cotangent ---------------------------------------------
def check_nan_filter(lib, dev, dtype_name="fp32", N=2, H=64, W=85):
    """MapNet++ step whose criterion emits NaN d(pred): with fc_wpqr = 0 every predicted log-quaternion is exactly zero,
    consecutive relative rotations are the identity and qlog_t's backward is inf * 0.  With
    filter_nans the reference zeroes the NaNs leaving fc_wpqr (grad of its input, weight, bias): the trunk then receives
    the translation path only.  HIP vs the oracle (real autograd + hooks): d(pred) NaN pattern, every parameter gradient,
    and -- without the filter -- NaN reaching the same parameters."""
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    out = {}
    for filt in (True, False):
        torch.manual_seed(7)
        onet = oracle.MapNet(oracle.PoseNet(oracle.resnet34(), droprate=0.0, pretrained=False, filter_nans=filt))
        with torch.no_grad():
            onet.mapnet.fc_wpqr.weight.zero_()
            onet.mapnet.fc_wpqr.bias.zero_()
        net = G.MapNet(G.PoseNet(G.resnet34(_binding=lib), droprate=0.0, pretrained=False, filter_nans=filt, _binding=lib))
        net.load_state_dict(onet.state_dict())
        if torch.device(dev).type == "cuda":
            net.cuda()
        x, t = oracle.make_batch("mapnet++", N, H, W, seed=7)
        oc = oracle.MapNetOnlineCriterion(0.0, -3.0, 0.0, -3.0, True, True)
        c = G.MapNetOnlineCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
        # lr = 0: the step leaves the weights alone, gradients stay inspectable on both sides
        oopt = oracle.Optimizer([{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}], "adam",
                                base_lr=0.0, weight_decay=0.0)
        opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                          base_lr=0.0, weight_decay=0.0)
        onet.train()
        net.train()
        lo, po = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True)
        l, p = G.step_feedfwd(x.to(dev), net, dev != "cpu", t.to(dev), c, opt, True)
        assert float(po.detach()[..., 3:].abs().max()) == 0.0 and float(p[..., 3:].abs().max()) == 0.0
        assert abs(l - lo) <= (1e-4 if dtype_name == "fp32" else 1e-2) * max(1.0, abs(lo)), (l, lo)
        eng = net.mapnet._engine
        plan = next(iter(eng.plans.values()))
        dpred = eng.debug_tensor(plan, "dposes").cpu().view(N, -1, 6)
        T = dpred.shape[1] // 2
        assert torch.isnan(dpred[:, T:, 3:]).all(), "the criterion's NaN cotangent did not appear"
        assert torch.isfinite(dpred[:, :T]).all() and torch.isfinite(dpred[:, T:, :3]).all()
        og = {k: v.grad for k, v in onet.mapnet.named_parameters()}
        worst, nan_names = 0.0, []
        for e in eng.entries:
            if e.is_buffer:
                continue
            name = e.name.decode()
            g = _view(eng.grads(), e).cpu().double()
            r = og[name].double()
            if not torch.isfinite(r).all():
                nan_names.append(name)
                assert not torch.isfinite(g).all(), (name, "oracle gradient is non-finite, HIP gradient is finite")
                continue
            assert torch.isfinite(g).all(), (name, "HIP gradient non-finite where the oracle's is finite", filt)
            if r.norm() < 1e-12:
                assert g.norm() < 1e-9, (name, g.norm())
            else:
                worst = max(worst, ((g - r).norm() / r.norm()).item())
        if filt:
            assert not nan_names, nan_names
            # fp16: at this batch size the ReLU network's gradient moves by tens of percent under fp16 rounding of the
            # activations (tools/layer_error.py: 0.3 relative at the full batch) -- finiteness and the zeroed tensors are
            # what the filter is about; the magnitudes are asserted in fp32
            assert worst <= (2e-2 if dtype_name == "fp32" else 1.0), worst
            g_w = _view(eng.grads(), next(e for e in eng.entries if e.name.decode() == "fc_wpqr.weight")).cpu()
            assert float(g_w.abs().max()) == 0.0  # NaN -> 0, as the hook does for the whole weight gradient
        else:
            assert "fc_wpqr.weight" in nan_names and "feature_extractor.conv1.weight" in nan_names, nan_names
        out[filt] = (worst, len(nan_names))
    return out


# ---- fp16 overflow: the step is skipped on the device, the host lowers the loss scale -----------------------------------
def check_debug_tensor_decodes_pair_layouts(lib, dev, N=1, H=32, W=40):
    """Engine.debug_tensor on the h2 / h2q tensors of the split-operand modes (dtype codes 3 / 5) returns VALUES, not the bytes of the
    pair layout viewed as floats (round-4 ADVICE): the first block's `a1` of an fp16x2 / fp16x2m / fp16x2q forward pass against the
    fp32 plan's on the same input and weights"""
    _fresh()
    import geomapnet_amd as G
    x, _ = oracle.make_batch("mapnet", N, H, W, seed=7)
    got = {}
    sd0 = None
    for dt in ("fp32", "fp16x2", "fp16x2m", "fp16x2q"):
        G.set_compute_dtype(dt)
        _, net = build_pair(lib, dev)
        if sd0 is None:
            sd0 = {k: v.clone() for k, v in net.state_dict().items()}
        else:
            net.load_state_dict(sd0)
        net.train()
        net(x.to(dev))
        eng = net.mapnet._engine
        plan = next(iter(eng.plans.values()))
        got[dt] = {n: eng.debug_tensor(plan, n).float().cpu().clone() for n in ("p0", "b0.a1", "b0.out")}
    for dt, tol in (("fp16x2", 1e-5), ("fp16x2m", 1e-5), ("fp16x2q", 5e-4)):
        for n, ref in got["fp32"].items():
            v = got[dt][n]
            assert v.shape == ref.shape, (dt, n, v.shape, ref.shape)
            err = ((v - ref).norm() / ref.norm()).item()
            assert err <= tol, (dt, n, err)


def check_overflow_skip(lib, dev, N=1, H=40, W=53, more=3, dtype_name="fp16"):
    """A loss scale far too large makes the fp16 activation gradients overflow: the step must leave parameters, Adam
    moments and the Adam step counter untouched (no inf/NaN anywhere), be counted, and the scale must come down; with a
    sane scale the next step is applied.  dtype_name fp16x2 / fp16x2m (the parity modes: their gradients pass through fp16 halves
    too): the first APPLIED step after the skipped ones must still be the oracle's first step to the north-star tolerance -- a
    skipped step may leave nothing behind (statistics, moments, step count) that bends the next one."""
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name, loss_scale=2.0 ** 60)
    try:
        onet, net = build_pair(lib, dev)
        c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
        opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                          base_lr=1e-3, weight_decay=5e-4)
        net.train()
        x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
        x, t = x.to(dev), t.to(dev)
        eng = net.mapnet._engine
        G.step_feedfwd(x, net, dev != "cpu", t, c, opt, True)
        dev_sync(dev)
        p0 = eng.params.clone()
        scale, skipped = eng.loss_scale_state()
        assert skipped == 1 and scale == 2.0 ** 60, (scale, skipped)
        sd = net.state_dict()
        assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype == torch.float32)
        assert float(eng.opt_state[eng.n_params:].abs().max()) == 0.0  # moments untouched
        assert not torch.isfinite(eng.grads()).all()                   # the overflow is in the gradients
        for _ in range(more):
            G.step_feedfwd(x, net, dev != "cpu", t, c, opt, True)
        dev_sync(dev)
        scale2, skipped2 = eng.loss_scale_state()
        assert skipped2 == 1 + more and scale2 < scale, (scale2, skipped2)   # the host has seen skips and halved
        assert torch.equal(eng.params[:-4], p0[:-4])
        assert opt.learner.state_dict()["state"] == {} or int(opt.learner.state_dict()["state"][0]["step"]) == 0
        plan = next(iter(eng.plans.values()))
        lib.check(lib.set_loss_scale(plan["handle"], C.c_float(1024.0), 0))
        l_rec, p_rec = G.step_feedfwd(x, net, dev != "cpu", t, c, opt, True)
        dev_sync(dev)
        assert eng.loss_scale_state() == (1024.0, 1 + more)
        if dtype_name != "fp16":  # the recovery step against the oracle's FIRST step (no step has been applied before it)
            oc = oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True)
            oopt = oracle.Optimizer([{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}],
                                    "adam", base_lr=1e-3, weight_decay=5e-4)
            onet.train()
            lo, po = oracle.step_feedfwd(x.cpu(), onet, False, t.cpu(), oc, oopt, True, 0.0)
            assert abs(l_rec - lo) <= 1e-4 * max(1.0, abs(lo)), (l_rec, lo)
            assert (p_rec.cpu() - po.detach()).abs().max().item() <= 1e-3
            # BatchNorm running statistics: the skipped forward passes DID update them (as the reference's would have: they are
            # not part of the optimiser step), so only finiteness is asserted for them; parameters must match the oracle's
            hp = dict(net.named_parameters())
            for k, v in onet.named_parameters():
                d_or = (v.detach() - hp[k].detach().cpu()).abs().max().item()
                assert d_or <= 2.5e-3, (k, d_or)  # lr 1e-3, sign-like first Adam update: a flipped sign costs 2 lr
        assert not torch.equal(eng.params[:-4], p0[:-4]) and torch.isfinite(eng.params).all()
        assert int(opt.learner.state_dict()["state"][0]["step"]) == 1
        # a second plan (another batch size, e.g. the last partial batch of an epoch) continues from the APPLIED count, not
        # from the number of attempts: Adam's bias corrections and the checkpointed `step` stay in agreement
        eng.loss_scale = 1024.0
        x2, t2 = oracle.make_batch("mapnet", N + 1, H, W, seed=8)
        G.step_feedfwd(x2.to(dev), net, dev != "cpu", t2.to(dev), c, opt, True)
        dev_sync(dev)
        assert len(eng.plans) == 2 and int(opt.learner.state_dict()["state"][0]["step"]) == 2
        G.step_feedfwd(x, net, dev != "cpu", t, c, opt, True)  # ... and back on the first plan
        assert int(opt.learner.state_dict()["state"][0]["step"]) == 3
    finally:
        G.set_compute_dtype("fp16", loss_scale=1024.0)


def check_overflow_progress_accounting(lib, dev, dtype_name="fp16", N=1, H=32, W=32):
    """The host's overflow bookkeeping (net.hip poll_overflow) must act on what the DEVICE reports as completed, not on polls that
    happened to see nothing new (round-4 ADVICE): (1) an isolated non-finite batch at loss scale 1 counts one stuck skip, polls that
    observe no newly completed attempt neither clear it nor advance the scale-growth counter, the next APPLIED step clears it;
    (2) the scale grows after `growth_interval` applied steps, not after that many polls; (3) permanently non-finite inputs at
    scale 1 keep counting and Engine.check_overflow_progress raises."""
    _fresh()
    import geomapnet_amd as G
    from geomapnet_amd._binding import MapNetHipError
    G.set_compute_dtype(dtype_name, loss_scale=1.0)
    try:
        _, net = build_pair(lib, dev)
        c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
        opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                          base_lr=1e-4, weight_decay=5e-4)
        net.train()
        x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
        x, t = x.to(dev), t.to(dev)
        bad = x.clone()
        bad[0, 0, 0, 0, 0] = float("nan")
        eng = net.mapnet._engine

        def step(inp):
            G.step_feedfwd(inp, net, dev != "cpu", t, c, opt, True)
            dev_sync(dev)

        step(x)  # creates the plan; applied
        plan = next(iter(eng.plans.values()))
        h = plan["handle"]
        stuck = lambda: int(lib.stuck_overflow_steps(h))  # noqa: E731
        lib.check(lib.set_loss_scale(h, C.c_float(1.0), 2))
        p_before = eng.params.clone()
        step(bad)  # skipped on the device; the host has not polled yet
        assert torch.equal(eng.params[:-4], p_before[:-4]) and eng.loss_scale_state() == (1.0, 1)
        assert stuck() == 0
        # polls WITHOUT a completed attempt in between: mn_train_forward_loss polls, runs a forward pass, applies nothing
        poses = torch.empty(plan["images"], 6, dtype=torch.float32, device=eng.device)
        for i in range(3):
            lib.check(lib.train_forward_loss(h, ptr(x), ptr(t.contiguous()), ptr(plan["loss"]), ptr(poses), None))
            dev_sync(dev)
            assert stuck() == 1, (i, stuck())                     # seen once, and NOT cleared by polls that observed nothing
            assert eng.loss_scale_state()[0] == 1.0, (i, eng.loss_scale_state())  # ... which do not count towards growth either
        step(x)   # applied (its own poll still saw nothing new: stuck stays 1 until the device reports the applied step)
        assert stuck() == 1
        step(x)   # this step's poll sees the applied attempt
        assert stuck() == 0
        # growth after 2 APPLIED steps (interval set above; the three polls above would have been enough for the old code): one of
        # them has completed and been seen so far
        assert eng.loss_scale_state()[0] == 1.0
        step(x)
        assert eng.loss_scale_state()[0] == 2.0, eng.loss_scale_state()
        # permanently non-finite inputs: the scale comes down to 1 first, then every further skip is a stuck one
        lib.check(lib.set_loss_scale(h, C.c_float(1.0), 0))
        raised = False
        try:  # (Engine._stepped samples the count every 16 steps: the raise may come from inside a step)
            for _ in range(9):
                step(bad)
            assert stuck() >= 8, stuck()
            eng.check_overflow_progress(plan)
        except MapNetHipError:
            raised = True
        assert raised and stuck() >= 8, "ten consecutive skipped steps at loss scale 1 must raise"
        try:
            step(x)
        except MapNetHipError:  # (the sampled check may fire once more before the applied step has been seen)
            pass
        step(x)
        step(x)
        assert stuck() == 0
    finally:
        G.set_compute_dtype("fp16", loss_scale=1024.0)


def check_deterministic(lib, dev, dtype_name, N=2, H=40, W=53, steps=3, max_grad_norm=5.0, repeat=True):
    """MN_DETERMINISTIC=1 (read when a plan is created): two runs of `steps` training steps from the same state are
    BIT-identical in parameters, Adam moments and loss -- BatchNorm sums through one accumulator row per producing
    workgroup, weight gradients through ordered slice / chunk reductions, the gradient norm through ordered partial sums --
    and the mode takes the same step as the default one up to the rounding of the summation order.  Returns the largest
    parameter difference between the two modes."""
    _fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    x, t = x.to(dev), t.to(dev)

    def run(det):
        old = os.environ.pop("MN_DETERMINISTIC", None)
        if det:
            os.environ["MN_DETERMINISTIC"] = "1"
        try:
            _, net = build_pair(lib, dev)
            c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
            opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                              base_lr=1e-4, weight_decay=5e-4)
            net.train()
            losses = []
            for _ in range(steps):
                loss, _ = G.step_feedfwd(x, net, dev != "cpu", t, c, opt, True, max_grad_norm=max_grad_norm)
                losses.append(float(loss))
            dev_sync(dev)
            eng = net.mapnet._engine
            return eng.params.clone().cpu(), eng.opt_state.clone().cpu(), losses
        finally:
            os.environ.pop("MN_DETERMINISTIC", None)
            if old is not None:
                os.environ["MN_DETERMINISTIC"] = old

    p1, o1, l1 = run(True)
    if repeat:  # (the emulator executes workgroups in order: nothing to reproduce there)
        p2, o2, l2 = run(True)
        assert torch.equal(p1, p2) and torch.equal(o1, o2) and l1 == l2, "deterministic mode is not reproducible"
    p0, o0, l0 = run(False)
    assert torch.isfinite(p1).all()
    # same step up to summation order: the first loss to 1e-4 (fp32) / 2e-3 (fp16); every further step amplifies the
    # summation-order difference ~30x (tools/oracle_sensitivity.py: the oracle against itself under another thread count)
    tol = 1e-4 if dtype_name == "fp32" else 2e-3
    for i, (a, b) in enumerate(zip(l0, l1)):
        assert abs(a - b) <= min(5e-2, tol * 30.0 ** i) * max(1.0, abs(a)), (l0, l1)
    return float((p0 - p1).abs().max())


# ---- BASELINE full-size parity against the oracle (all three modes) ----------------------------------------------------
# What fp16 STORAGE costs at the 64-window shapes, i.e. the deviation of the oracle from itself when the tensors the fp16
# build keeps in fp16 are rounded (profiles/r02/fp16_budget_cpu.txt: pose 1.29e-2 max; profiles/r03/
# fp16_budget_backward_cpu.txt: gradients), and the largest values measured on MI355X over the three BASELINE shapes
# (profiles/r02/parity_full_size.jsonl: loss 7.9e-4, pose 1.44e-2, gradients 0.158 overall / 0.389 worst tensor), x 1.5.
# The fp16 mode at the SMALL shapes of the suite (round 6): 1.5x what the mode measures on MI355X at each
# shape (profiles/r06/c3_fp16_deviation_at_the_suite_shapes.txt) -- a 3x regression of the fast mode used to pass the 1e-2 / 3e-2 /
# unchecked-gradient gates.  key = (N, H, W): first-step loss (relative), pose (max abs), worst-tensor gradient (relative L2), and the
# second step's (loss, pose) where two steps are taken (Adam's sign-like first update amplifies the first step's deviation ~30x).
FP16_SMALL = {
    (2, 64, 85): {"loss": 1.5 * 7.74e-4, "pose": 1.5 * 2.04e-2, "grad": 1.5 * 0.340, "later": (1.5 * 5.53e-3, 1.5 * 0.214),
                  "crit": 1.5 * 4.0e-3},
    (2, 256, 341): {"loss": 1.5 * 6.88e-4, "pose": 1.5 * 9.55e-3, "grad": 1.5 * 0.355, "later": None, "crit": 1.5 * 2.3e-3},
}


def fp16_small_gates(N, H, W):
    """keyword arguments of check_train_step for the fp16 mode at a suite shape"""
    e = FP16_SMALL[(N, H, W)]
    return {"loss_rtol": e["loss"], "pose_atol": e["pose"], "grad_l2_rtol": e["grad"], "later_tol": e["later"],
            "crit_grad_rtol": e["crit"]}


FP16_ENVELOPE = {"loss_rel": 1.2e-3, "pose_abs_max": 2.2e-2, "grad_l2_rel_all": 0.25, "grad_l2_rel_worst_tensor": 0.6}



def check_full_size_parity(lib, dev, mode, N, H=256, W=341, max_grad_norm=0.0, lr=1e-4, wd=5e-4, filter_nans=False,
                           fp32_loss_rtol=1e-4, fp32_pose_atol=1e-3):
    """One training step of a BASELINE.json configuration at FULL size: oracle (CPU fp32) once, then HIP in fp32x3 (the
    parity mode on the f16 / bf16 matrix pipe) and fp32, both asserted to the north-star bar as written -- 1e-4 on loss
    relative to max(1,|loss|), 1e-3 on pose (max abs) -- and in fp16, asserted to stay within 1.5x of what its storage
    format costs the ORACLE (tools/fp16_budget.py, tools/fp16_budget_backward.py replay the oracle with fp16 rounding at
    the build's storage points: FP16_ENVELOPE below).  Returns the measurements."""
    _fresh()
    import time
    import geomapnet_amd as G
    torch.manual_seed(7)
    onet = oracle.MapNet(oracle.PoseNet(oracle.resnet34(), droprate=0.0, pretrained=False, filter_nans=filter_nans))
    sd0 = {k: v.clone() for k, v in onet.state_dict().items()}
    x, t = oracle.make_batch(mode, N, H, W, seed=7)
    if mode == "posenet":
        omodel = onet.mapnet
        oc = oracle.PoseNetCriterion(0.0, -3.0, True)
        og = [{"params": omodel.parameters()}, {"params": [oc.sax, oc.saq]}]
    else:
        omodel = onet
        oc = (oracle.MapNetCriterion(0.0, -3.0, 0.0, -3.0, True, True) if mode == "mapnet"
              else oracle.MapNetOnlineCriterion(0.0, -3.0, 0.0, -3.0, True, True))
        og = [{"params": omodel.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}]
    oopt = oracle.Optimizer(og, "adam", base_lr=lr, weight_decay=wd)
    omodel.train()
    t0 = time.time()
    lo, po = oracle.step_feedfwd(x, omodel, False, t, oc, oopt, True, max_grad_norm)
    oracle_s = time.time() - t0
    po = po.detach()
    ograd = {k: v.grad.clone() for k, v in onet.mapnet.named_parameters()}
    frames = x.shape[1] if x.dim() == 5 else 1
    rec = {"mode": mode, "windows": N, "images": N * frames, "H": H, "W": W, "oracle_step_s": round(oracle_s, 1),
           "loss_oracle": lo, "pose_scale": po.abs().max().item()}
    del omodel, oopt
    for dtype_name in ("fp16x2m", "fp16x2", "fp16x2q", "fp32x3", "fp32", "fp16"):
        G.set_compute_dtype(dtype_name)
        net = G.MapNet(G.PoseNet(G.resnet34(_binding=lib), droprate=0.0, pretrained=False, filter_nans=filter_nans, _binding=lib))
        net.load_state_dict(sd0)
        if torch.device(dev).type == "cuda":
            net.cuda()
        if mode == "posenet":
            model = net.mapnet
            c = G.PoseNetCriterion(sax=0.0, saq=-3.0, learn_beta=True, _binding=lib)
            gg = [{"params": model.parameters()}, {"params": [c.sax, c.saq]}]
        else:
            model = net
            c = (G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
                 if mode == "mapnet" else
                 G.MapNetOnlineCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib))
            gg = [{"params": model.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}]
        opt = G.Optimizer(gg, "adam", base_lr=lr, weight_decay=wd)
        model.train()
        l, p = G.step_feedfwd(x.to(dev), model, dev != "cpu", t.to(dev), c, opt, True, max_grad_norm)
        d = p.cpu() - po
        eng = net.mapnet._engine
        num = den = 0.0
        worst = 0.0
        mine = {}
        for e in eng.entries:
            if e.is_buffer:
                continue
            g = _view(eng.grads(), e).cpu().double()
            mine[e.name.decode()] = g.clone()
            r = ograd[e.name.decode()].double()
            if max_grad_norm > 0.0:
                continue  # the oracle's stored gradients are already clipped, the arena's are not
            num += (g - r).pow(2).sum().item()
            den += r.pow(2).sum().item()
            if r.norm() > 1e-8:
                worst = max(worst, ((g - r).norm() / r.norm()).item())
        rec[dtype_name] = {"loss": l, "loss_rel": abs(l - lo) / max(1.0, abs(lo)), "pose_abs_max": d.abs().max().item(),
                           "pose_abs_rms": d.pow(2).mean().sqrt().item(),
                           "grad_l2_rel_all": (num / den) ** 0.5 if den > 0 else None, "grad_l2_rel_worst_tensor": worst}
        if dtype_name in ("fp16x2m", "fp16x2"):  # the two arenas against each other (unclipped on both sides)
            if dtype_name == "fp16x2m":
                mixed_grads = mine
            else:
                n2 = d2 = w2 = 0.0
                for k, g2 in mine.items():
                    n2 += (mixed_grads[k] - g2).pow(2).sum().item()
                    d2 += g2.pow(2).sum().item()
                    if g2.norm() > 1e-8:
                        w2 = max(w2, ((mixed_grads[k] - g2).norm() / g2.norm()).item())
                rec["fp16x2m"]["grad_vs_fp16x2_all"] = (n2 / d2) ** 0.5
                rec["fp16x2m"]["grad_vs_fp16x2_worst_tensor"] = w2
                del mixed_grads
        del net, model, opt, c
    # fp16x2m (round 5): the fp16x2 forward pass, so its loss and poses must be that mode's BITS; its single-fp16 backward pass is
    # held to the same gradient bars as the fp32-class modes and, directly, to 3e-3 / 6e-3 of fp16x2's gradients -- operand
    # rounding only (tools/mixed_budget.py: 6.4e-4 / 1.6e-3 from the oracle's own arithmetic), where a gate or a BatchNorm statistic
    # taken from a rounded forward value would show as percents
    assert rec["fp16x2m"]["loss"] == rec["fp16x2"]["loss"] and rec["fp16x2m"]["pose_abs_max"] == rec["fp16x2"]["pose_abs_max"], rec
    if rec["fp16x2m"].get("grad_vs_fp16x2_all") is not None:
        assert rec["fp16x2m"]["grad_vs_fp16x2_all"] <= 3e-3 and rec["fp16x2m"]["grad_vs_fp16x2_worst_tensor"] <= 6e-3, rec
    for name in ("fp16x2m", "fp16x2", "fp32x3", "fp32"):
        assert rec[name]["loss_rel"] <= fp32_loss_rtol, (name, rec)
        assert rec[name]["pose_abs_max"] <= fp32_pose_atol, (name, rec)
        if rec[name]["grad_l2_rel_all"] is not None:  # (gate flips: DESIGN.md section 6)
            assert rec[name]["grad_l2_rel_all"] <= 2e-2 and rec[name]["grad_l2_rel_worst_tensor"] <= 5e-2, (name, rec)
    # fp16x2q (experimental: fp8 cross terms in the forward convolutions): the POSES stay inside the north-star bar and the loss inside
    # its relative reading, at a margin of 1.5-2.5x instead of fp16x2m's 60x; the gradients are off by percents (the 1e-4-relative forward
    # error moves ReLU gates and BatchNorm statistics: measured 2.9 % / 6.8 % at configs[2]) -- between fp16x2m (0.5 % / 1.3 %) and fp16
    # (15.8 % / 38.9 %): NOT a parity mode
    q = rec["fp16x2q"]
    assert q["loss_rel"] <= 1e-4 and q["pose_abs_max"] <= 1e-3, rec
    if q["grad_l2_rel_all"] is not None:
        assert q["grad_l2_rel_all"] <= 0.06 and q["grad_l2_rel_worst_tensor"] <= 0.15, rec
    env = FP16_ENVELOPE
    assert rec["fp16"]["loss_rel"] <= env["loss_rel"] and rec["fp16"]["pose_abs_max"] <= env["pose_abs_max"], rec
    if rec["fp16"]["grad_l2_rel_all"] is not None:
        assert rec["fp16"]["grad_l2_rel_all"] <= env["grad_l2_rel_all"], rec
        assert rec["fp16"]["grad_l2_rel_worst_tensor"] <= env["grad_l2_rel_worst_tensor"], rec
    return rec


def check_loss_trajectory(lib, dev, N=8, H=256, W=341, steps=50, lr=1e-4, envelope=0.25, modes=("fp16", "fp32x3"), extra=()):
    """(modes = (tested, reference); `extra`: further modes whose curves are only recorded, with their gap to the reference.)
    Does the fp16 build TRAIN like the parity mode?  Two HIP models (fp16 and fp32x3), identical initial weights and one
    fixed batch, `steps` Adam steps each on the same device; the loss curves are compared point by point, relative to
    the total descent of the fp32x3 curve.  (Single steps are pinned against the oracle elsewhere; steps after the first
    can only be compared loosely -- Adam's first updates are sign-like and the random-init network amplifies any
    difference ~30x per step, DESIGN.md section 6 -- so this is an envelope on the whole trajectory.)
    Returns (fp16 losses, fp32x3 losses, largest pointwise gap / descent)."""
    _fresh()
    import geomapnet_amd as G
    torch.manual_seed(7)
    onet = oracle.MapNet(oracle.PoseNet(oracle.resnet34(), droprate=0.0, pretrained=False))
    sd0 = {k: v.clone() for k, v in onet.state_dict().items()}
    del onet
    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    x, t = x.to(dev), t.to(dev)
    curves = {}
    for dtype_name in tuple(modes) + tuple(extra):
        G.set_compute_dtype(dtype_name)
        net = G.MapNet(G.PoseNet(G.resnet34(_binding=lib), droprate=0.0, pretrained=False, _binding=lib))
        net.load_state_dict(sd0)
        if torch.device(dev).type == "cuda":
            net.cuda()
        c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
        opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                          base_lr=lr, weight_decay=5e-4)
        net.train()
        curves[dtype_name] = [G.step_feedfwd(x, net, dev != "cpu", t, c, opt, True)[0] for _ in range(steps)]
        del net, c, opt
    a, b = np.array(curves[modes[0]]), np.array(curves[modes[1]])
    assert np.isfinite(a).all() and np.isfinite(b).all()
    descent = b[0] - b.min()
    assert descent > 0.5 * abs(b[0]), (b[0], b.min())  # the fixed batch is being fitted
    gap = float(np.abs(a - b).max() / descent)
    assert gap <= envelope, (gap, curves)
    if extra:
        return curves, gap, {e: float(np.abs(np.array(curves[e]) - b).max() / descent) for e in extra}
    return curves[modes[0]], curves[modes[1]], gap


def check_dense(lib, dev, B, Cin, F, seed=11):
    """the pose head's dense layer (csrc/dense.h): forward with bias + ReLU, data gradient (the same kernel against the transposed
    weight), weight + bias gradient (`+=` onto a non-zero start), and the pose regressors' weight gradient with the NaN filter, each
    against torch in fp64 at fp32 round-off (exact fp32 products, sums in a different order)"""
    _fresh()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, generator=gen)
    w = torch.randn(F, Cin, generator=gen) * 0.05
    bias = torch.randn(F, generator=gen) * 0.1
    ref = torch.relu(x.double() @ w.double().t() + bias.double())
    out = torch.full((B, F), float("nan"), device=dev)
    lib.check(lib.op_dense(K(x.to(dev)), K(w.to(dev)), K(bias.to(dev)), K(out), B, F, Cin, 1, None))
    dev_sync(dev)
    assert (out.cpu().double() - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())
    dz = torch.randn(B, F, generator=gen)
    if F % 128 == 0:  # data gradient: dz . W = dz . (W^T)^T
        wt = w.t().contiguous()
        gx = torch.full((B, Cin), float("nan"), device=dev)
        lib.check(lib.op_dense(K(dz.to(dev)), K(wt.to(dev)), None, K(gx), B, Cin, F, 0, None))
        dev_sync(dev)
        rgx = dz.double() @ w.double()
        assert (gx.cpu().double() - rgx).abs().max().item() <= 2e-6 * max(1.0, rgx.abs().max().item())
    dw0, db0 = torch.randn(F, Cin, generator=gen), torch.randn(F, generator=gen)
    dw, db = dw0.clone().to(dev), db0.clone().to(dev)
    alpha = 0.25
    lib.check(lib.op_dense_wgrad(K(dz.to(dev)), K(x.to(dev)), K(dw), K(db), B, F, Cin, f32(alpha), None))
    dev_sync(dev)
    rdw = dw0.double() + alpha * (dz.double().t() @ x.double())
    rdb = db0.double() + alpha * dz.double().sum(0)
    assert (dw.cpu().double() - rdw).abs().max().item() <= 2e-6 * max(1.0, rdw.abs().max().item())
    assert (db.cpu().double() - rdb).abs().max().item() <= 2e-6 * max(1.0, rdb.abs().max().item())
    # pose regressors: feat [B][F], dposes [B][6], a NaN in the rotation part of one row
    feat = torch.relu(torch.randn(B, F, generator=gen))
    dp = torch.randn(B, 6, generator=gen)
    for filt in (0, 1):
        dpn = dp.clone()
        if filt:
            dpn[B // 2, 4] = float("nan")
        bufs = [torch.zeros(3, F, device=dev), torch.zeros(3, device=dev), torch.zeros(3, F, device=dev), torch.zeros(3, device=dev)]
        for t in bufs:
            t.fill_(0.5)
        lib.check(lib.op_head_wgrad(K(dpn.to(dev)), K(feat.to(dev)), K(bufs[0]), K(bufs[1]), K(bufs[2]), K(bufs[3]), B, F, f32(alpha),
                                    filt, None))
        dev_sync(dev)
        rx = 0.5 + alpha * (dpn[:, :3].double().t() @ feat.double())
        rq = 0.5 + alpha * (dpn[:, 3:].double().t() @ feat.double())
        rbx, rbq = 0.5 + alpha * dpn[:, :3].double().sum(0), 0.5 + alpha * dpn[:, 3:].double().sum(0)
        if filt:  # filter_hook: NaN entries of the rotation regressor's gradients become 0 before they are accumulated
            rq = torch.where(torch.isnan(rq), torch.full_like(rq, 0.5), rq)
            rbq = torch.where(torch.isnan(rbq), torch.full_like(rbq, 0.5), rbq)
        for got, want in zip(bufs, (rx, rbx, rq, rbq)):
            assert (got.cpu().double() - want).abs().max().item() <= 5e-6 * max(1.0, want.abs().max().item())


def check_stem_bwd(lib, dev, B, H, W, seed=5, pre_gated=False):
    """stem backward in two launches (csrc/stem_bwd.h: BatchNorm sums with the max-pool gradient gathered on the fly, then the
    weight gradient with d(conv output) computed in LDS), two ways: (1) SELF-CONSISTENCY against the four-launch chain of
    the operators it replaces (maxpool_bwd -> bn_bwd -> wgrad) on identical fp16 tensors -- same arithmetic, same
    roundings, tight tolerance; (2) DIRECTLY against torch autograd in fp64 through maxpool(relu(batchnorm(y))) and the
    convolution's weight gradient (d(weight), d(gamma), d(beta)) at the tolerance of the fp16 tensors involved.
    pre_gated (mn_op_stem_bwd_pregated, the fp16x2m mode): the pooled gradient arrives already gated and the kernels must NOT gate it
    again by the ReLU recomputed from y.  The mask applied to gp here is random, i.e. unrelated to the sign y gives -- as the exact gate
    of the fp32 forward pass is for the few values whose fp16 copy falls on the other side of the threshold, only everywhere -- so a
    kernel that recomputed the gate is wrong by O(1); both references then take the gathered gradient as it is (no ReLU gate)."""
    _fresh()
    td = torch.float16
    gen = torch.Generator().manual_seed(seed)
    g, Hp, Wp, H0, W0 = stem_geom(B, H, W)
    Po, Qo = (H0 - 1) // 2 + 1, (W0 - 1) // 2 + 1
    x = torch.randn(B, 3, H, W, generator=gen).to(td).float()
    xp = torch.zeros(B, Hp, Wp, 4)
    xp[:, 3:3 + H, 3:3 + W, :3] = x.permute(0, 2, 3, 1)
    xp = xp.to(td).to(dev)
    y = (torch.randn(B, H0, W0, 64, generator=gen) * 1.5 + 0.3).to(td).to(dev)  # stands for the raw conv output
    gamma = (1.0 + 0.2 * torch.randn(64, generator=gen)).to(dev)
    beta = (0.1 * torch.randn(64, generator=gen)).to(dev)
    M = B * H0 * W0
    mean, invstd = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    a0 = torch.zeros(B, H0, W0, 64, dtype=td, device=dev)
    scratch = torch.zeros(2 * 64 * 8 + 2 * 64 * 4, dtype=torch.uint8, device=dev)
    rm, rv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    lib.check(lib.op_bn_train_fwd(1, K(y), M, 64, K(gamma), K(beta), K(rm), K(rv), K(mean), K(invstd), None, 1, K(a0), f32(1e-5),
                                  f32(0.1), K(scratch), None))
    p0 = torch.zeros(B, Po, Qo, 64, dtype=td, device=dev)
    idx = torch.zeros(B, Po, Qo, 64, dtype=torch.uint8, device=dev)
    lib.check(lib.op_maxpool_fwd(1, K(a0), K(p0), K(idx), B, H0, W0, 64, None))
    gp = torch.randn(B, Po, Qo, 64, generator=gen).to(td).to(dev)
    if pre_gated:
        gp = gp * (torch.rand(B, Po, Qo, 64, generator=gen) < 0.5).to(td).to(dev)
    cm = torch.full((224,), -1, dtype=torch.int32)
    for r in range(7):
        for s4 in range(4):
            for e in range(8):
                sp, ch = 2 * s4 + (e >> 2), e & 3
                if sp < 7 and ch < 3:
                    cm[(r * 4 + s4) * 8 + e] = (r * 7 + sp) * 3 + ch
    cm = cm.to(dev)
    alpha = 1.0 / 64.0
    # the chain it replaces
    ga0 = torch.zeros(B, H0, W0, 64, dtype=td, device=dev)
    lib.check(lib.op_maxpool_bwd(1, K(idx), K(gp), K(ga0), B, H0, W0, 64, None))
    dg_ref, db_ref = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    gy = torch.zeros(B, H0, W0, 64, dtype=td, device=dev)
    coef = torch.zeros(4 * 64, device=dev)
    acc = torch.zeros(2 * 64, dtype=torch.float64, device=dev)
    lib.check(lib.op_bn_bwd(1, K(ga0), None if pre_gated else K(a0), K(y), M, 64, K(gamma), K(mean), K(invstd), K(dg_ref), K(db_ref),
                            K(gy), K(coef), K(acc), f32(alpha), None))
    dW_ref = torch.zeros(64, 147, device=dev)
    lib.check(lib.op_wgrad(1, C.byref(g), K(gy), 64, K(xp), K(dW_ref), 147, K(cm), f32(alpha), 16, K(zero_page(dev)), None))
    # the two-launch form
    dg, db = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    dW = torch.zeros(64, 147, device=dev)
    coef2 = torch.zeros(4 * 64, device=dev)
    acc2 = torch.zeros(2 * 64, dtype=torch.float64, device=dev)
    op = lib.op_stem_bwd_pregated if pre_gated else lib.op_stem_bwd
    lib.check(op(K(y), K(idx), K(gp), K(gamma), K(beta), K(mean), K(invstd), K(xp), K(dW), 147, K(cm), K(dg), K(db),
                 K(coef2), K(acc2), B, H, W, Wp, f32(alpha), None))
    dev_sync(dev)
    scale = dW_ref.abs().max().item()
    assert scale > 0
    self_err = (dW - dW_ref).abs().max().item()
    if not pre_gated:
        assert self_err <= 2e-4 * scale, (self_err, scale)
    # d(gamma), d(beta): the chain sums the max-pool's input gradient as STORED (a pixel that is the argmax of several
    # windows holds their sum rounded to fp16); stem_bn_reduce_kernel walks the windows and adds every window's fp16
    # gradient to its fp32 sums unrounded -- the two differ by that rounding (5e-4 relative on the affected pixels), the
    # window-order sums being the ones closer to exact arithmetic (part 2 below)
    np.testing.assert_allclose(dg.cpu().numpy(), dg_ref.cpu().numpy(), rtol=1e-3, atol=1e-3 * float(dg_ref.abs().max()))
    np.testing.assert_allclose(db.cpu().numpy(), db_ref.cpu().numpy(), rtol=1e-3, atol=1e-3 * float(db_ref.abs().max()))
    # (2) torch fp64 on the same (fp16-representable) inputs: y is a leaf standing for the conv output
    y64 = y.cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    g64 = gamma.cpu().double().requires_grad_(True)
    b64 = beta.cpu().double().requires_grad_(True)
    a64 = F.batch_norm(y64, None, None, g64, b64, True, 0.0, 1e-5)
    if not pre_gated:
        a64 = F.relu(a64)
    # the kernel's max-pool routes through the fp16-rounded activation (first maximum wins).  Distinct fp64 values that
    # round to one fp16 value are NOT rare at full resolution (4.2 M windows; the first GPU run of this comparison at
    # 3 x 256 x 341 was 1.4 % off in d(weight) from such ties alone), so the argmax is taken on the stored fp16
    # activation a0 -- the tensor the forward kernel compared -- and the fp64 values are gathered through it
    a16 = a0.cpu().double().permute(0, 3, 1, 2).contiguous()
    _, pidx = F.max_pool2d(a16, 3, 2, 1, return_indices=True)
    p64 = a64.flatten(2).gather(2, pidx.flatten(2)).view_as(pidx)
    p64.backward(gp.cpu().double().permute(0, 3, 1, 2).contiguous())
    gy64 = y64.grad  # d(conv output)
    dW64 = torch.nn.grad.conv2d_weight(x.double(), (64, 3, 7, 7), gy64, stride=2, padding=3) * alpha
    dW_t = dW.cpu().double().reshape(64, 7, 7, 3).permute(0, 3, 1, 2)  # [64][r][s][c] -> OIHW
    s64 = dW64.abs().max().item()
    assert (dW_t - dW64).abs().max().item() <= 4e-3 * s64, ((dW_t - dW64).abs().max().item(), s64)
    if pre_gated:
        # (1) for the pre-gated form: a bar per element of dW, derived from what may differ between the two forms.  Both compute
        #   gy = fp16(k1 (gm - mg - xhat mgx))  from the same gm, k1 and xhat; they differ in the sums (mg, mgx), taken in another order.
        # The d(beta) / d(gamma) assertions above hold those to 1e-3 (|v| + max|v|), i.e. dmg, dmgx below that over alpha M.  Before
        # rounding the two gy then differ by at most d = k1 (dmg + |xhat| dmgx); after rounding by d plus, where a rounding boundary
        # lies inside that interval -- probability p = min(1, d / ulp) -- one fp16 ulp of gy, with either sign, independently per
        # element.  dW = alpha sum_m gy x, so  |dW - dW_ref| <= alpha (sum d |x| + 6 sqrt(sum p ulp^2 x^2)) + 1e-6 max|dW|
        # (six standard deviations of the flips; the last term: fp32 accumulation in another order).  Without the ReLU gate about
        # twice as many pixels carry gradient as in the gated form, which is why the flat 2e-4 of that form is not carried over
        # (at 140 pixels either form exceeds it for one seed in three).  A kernel that gated again by the recomputed ReLU is off by O(1).
        cnt = alpha * M
        dgr, dbr = dg_ref.cpu().double(), db_ref.cpu().double()
        dmgx = 1e-3 * (dgr.abs() + dgr.abs().max()) / cnt
        dmg = 1e-3 * (dbr.abs() + dbr.abs().max()) / cnt
        k1 = (gamma.cpu().double() * invstd.cpu().double()).abs()
        xhat = ((y.cpu().double() - mean.cpu().double()) * invstd.cpu().double()).abs()
        gyc = gy.cpu().double().abs()
        d = k1 * (dmg + xhat * dmgx)
        ulp = torch.clamp(2.0 ** (torch.floor(torch.log2(torch.clamp(gyc, min=2.0 ** -14))) - 10), min=2.0 ** -24)
        pflip = torch.clamp(d / ulp, max=1.0)
        nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()  # noqa: E731
        cw = lambda xin, gin: torch.nn.grad.conv2d_weight(xin, (64, 3, 7, 7), nchw(gin), stride=2, padding=3)  # noqa: E731
        bar = alpha * (cw(x.double().abs(), d) + 6.0 * torch.sqrt(cw(x.double() ** 2, pflip * ulp ** 2))) + 1e-6 * scale
        dW_r = dW_ref.cpu().double().reshape(64, 7, 7, 3).permute(0, 3, 1, 2)
        worst = ((dW_t - dW_r).abs() / bar).max().item()
        if os.environ.get("MN_PRINT_FIGURES"):
            print("pre-gated stem: |dW - chain| / bar = %.3f, bar / max|dW| = %.2e .. %.2e" % (worst, (bar / scale).min().item(), (bar / scale).max().item()))
        assert worst <= 1.0, ("two-launch form vs the chain / derived bar", worst)
    np.testing.assert_allclose(dg.cpu().double().numpy(), (g64.grad * alpha).numpy(), rtol=0, atol=4e-3 * float(g64.grad.abs().max() * alpha))
    np.testing.assert_allclose(db.cpu().double().numpy(), (b64.grad * alpha).numpy(), rtol=0, atol=4e-3 * float(b64.grad.abs().max() * alpha))


def check_device_feed(lib, dev, dtype_name="fp16", N=8, H=256, W=341, batches=6, u8=False, staged_env=None):
    """geomapnet_amd.DeviceFeed (the copy of batch k+1 on a copy stream under step k, rotating staging buffers) against the same
    batches copied synchronously in front of each step, under MN_DETERMINISTIC=1 -- every step is bit-reproducible there, so ONE
    staging buffer overwritten while a step still reads it, or a step started before its copy has landed, changes the bits of a loss
    or of the final parameters.  The batches are distinct and large (the copy of batch k+1 spans a good part of step k); `batches` >
    2 x depth so every staging slot is reused several times.  staged_env: extra environment for the second run (the staged
    data-parallel step with the stand-in collective and a deferred-bucket schedule must compute the same bits as well)."""
    _fresh()
    import geomapnet_amd as G
    import geomapnet_amd.train as T
    G.set_compute_dtype(dtype_name)
    gen = torch.Generator().manual_seed(3)
    cuda = torch.device(dev).type == "cuda"

    def pin(t):
        return t.pin_memory() if cuda else t

    if u8:
        xs = [pin(torch.randint(0, 256, (N, 3, H, W, 3), generator=gen, dtype=torch.uint8)) for _ in range(batches)]
    else:
        xs = [pin(torch.randn(N, 3, 3, H, W, generator=gen)) for _ in range(batches)]
    ts = [pin(torch.randn(N, 3, 6, generator=gen) * 0.3) for _ in range(batches)]

    def run(feed, env=None):
        old = {k: os.environ.get(k) for k in ["MN_DETERMINISTIC"] + list(env or {})}
        os.environ["MN_DETERMINISTIC"] = "1"
        os.environ.update(env or {})
        forced = T._FORCE_STAGED
        if env and env.get("MN_FORCE_STAGED") == "1":
            T._FORCE_STAGED = True
        try:
            _, net = build_pair(lib, dev)
            if u8:
                net.set_input_u8((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
            c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
            opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                              base_lr=1e-4, weight_decay=5e-4)
            net.train()
            losses = []
            if feed:
                src = G.DeviceFeed(list(zip(xs, ts)), dev)
            else:
                src = ((x.to(dev), t.to(dev)) for x, t in zip(xs, ts))
            for x, t in src:
                if not feed:
                    dev_sync(dev)  # the copy has landed before the step is enqueued
                loss, _ = G.step_feedfwd(x, net, cuda, t, c, opt, True)
                losses.append(float(loss))
            dev_sync(dev)
            eng = net.mapnet._engine
            return losses, eng.params.clone().cpu()
        finally:
            T._FORCE_STAGED = forced
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v

    l0, p0 = run(False)
    l1, p1 = run(True, staged_env)
    assert all(v == v for v in l0) and len(set(l0)) == len(l0), l0  # finite, and the batches really differ
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    return l0
