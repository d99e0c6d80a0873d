"""Backend-agnostic checks of the fused inference pass (csrc/igemm.h Epilogue::bn_coef and the EV instantiations of the three h2
forward kernels, mn_op_conv_bn_eval, mn_set_eval_fused): each takes a Binding (`lib`) and a torch device, so the CPU suite runs them
on the SIMT-emulator build and the GPU suite on libmapnet_hip.so.

Which layer1 form ships: the fused instantiation of conv_halo_h2_kernel (halo_h2.h) has no scratch, so layer1 runs it and the
plan-level bit equality below covers layer1 too; igemm_halo_kernel<64, 368, A1> is not a fallback of the fused path."""
import ctypes as C

import torch
import torch.nn.functional as F

import checks
import oracle
from checks import K, from_h2, h2_value, to_h2

H2 = 3  # MN_DTYPE_F16X2
SENTINEL = 777.0  # poison of `out`: no half of a written element can hold it (outputs are O(10), lo halves below 2^-10 of them)

# (B, H, W, Cin, Cout, k, stride, pad): the smallest shapes that reach each instantiation with ragged tiles.  The dispatcher's
# conditions (igemm.h launch_igemm_h2, igemm_halo.h launch_igemm_halo_h2) evaluated for each, 256 compute units:
# conv_halo_h2_kernel: 64 -> 64 channels, 3x3 stride 1; one partial 8x16 tile per image / several tiles in both directions, all ragged
HALO_H2_SHAPES = ((2, 9, 11, 64, 64, 3, 1, 1), (1, 17, 33, 64, 64, 3, 1, 1))
# igemm_kernel<half, ..., MMA_H2>, 128x128 tiles of four waves: stride-2 3x3 and the 1x1 stride-2 projections.  (The h2 dispatcher
# has no 288x256 configuration of igemm_kernel and does not read MN_IGEMM_CONFIG, so there is no forced tile to cover: the last shape,
# 256 columns at stride 2, is one of the two the issue lists for that knob and runs on this tile, as its unfused launch does.)
IGEMM_SHAPES = ((2, 9, 11, 64, 128, 3, 2, 1), (2, 8, 10, 64, 128, 1, 2, 0), (2, 7, 9, 64, 128, 1, 2, 0), (2, 16, 22, 256, 512, 1, 2, 0),
                (2, 18, 22, 64, 256, 3, 2, 1))
# igemm_kernel<half, ..., MMA_H2>, the 128x64 tile (N <= 64; no convolution of the network takes it, the operator does): a ragged
# 64-column projection, and 40 columns in h2 rows of 64 (ldc > N, the last 32-channel group a quarter full)
IGEMM64_SHAPES = ((2, 7, 9, 64, 64, 1, 2, 0), (2, 7, 9, 64, 40, 1, 2, 0))
# igemm_halo <64, 368, A1>: 64 columns, 3x3 stride 1, with other than 64 input channels (those go to conv_halo_h2_kernel)
HALO64_SHAPES = ((2, 9, 11, 128, 64, 3, 1, 1),)
# igemm_halo <128, 480, 4x2 waves>: the default at small sizes (384-row tiles fill the chip's rounds as well as 288-row tiles); the
# last shape, 256 columns, is the other one the issue lists under MN_IGEMM_CONFIG=12
HALO480_SHAPES = ((3, 9, 11, 64, 128, 3, 1, 1), (2, 12, 43, 128, 128, 3, 1, 1), (4, 8, 11, 512, 512, 3, 1, 1), (4, 9, 11, 64, 256, 3, 1, 1))
# igemm_halo <128, 288, A1> under MN_HALO_A1=2
A1_SHAPES = ((2, 12, 43, 128, 128, 3, 1, 1), (40, 3, 5, 64, 128, 3, 1, 1))
# igemm_halo <256, 352> under MN_H2_HALO256=1
HALO256_SHAPES = ((3, 16, 22, 256, 256, 3, 1, 1), (2, 13, 31, 192, 256, 3, 1, 1))
# igemm_halo <128, 384>: 140 tiles of 384 rows fill 0.55 of a round, 184 of 288 rows 0.72 -- the e384 / e288 rule picks 288 rows
HALO384_SHAPES = ((150, 8, 11, 512, 512, 3, 1, 1),)
# hundreds of concurrent workgroups (race screen; once each, residual and ReLU on)
RACE_SHAPES = ((48, 32, 43, 128, 128, 3, 1, 1), (96, 16, 22, 256, 256, 3, 1, 1))


def conv_operands(lib, dev, shape, seed=0):
    """x, w, the fp64 convolution of their h2 values and the unfused device convolution (mn_op_igemm dtype 3) of one shape: computed
    once, shared by the four (residual, ReLU) variants, never written again"""
    B, H, W, Cin, Cout, k, stride, pad = shape
    gen = torch.Generator().manual_seed(seed)
    x = h2_value(torch.randn(B, Cin, H, W, generator=gen))
    w = h2_value(torch.randn(Cout, Cin, k, k, generator=gen) * (2.0 / (Cin * k * k)) ** 0.5)
    conv64 = F.conv2d(x.double(), w.double(), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()  # [B][Ho][Wo][Cout]
    g, Ho, Wo = checks.fwd_geom(*shape)
    xn, wn = to_h2(x.permute(0, 2, 3, 1)).to(dev), to_h2(w.permute(0, 2, 3, 1)).to(dev)
    y = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float32, device=dev)
    lib.check(lib.op_igemm(H2, C.byref(g), K(xn), K(wn), K(y), Cout, None, None, 0, None, None, checks.f32(1), K(checks.zero_page(dev)),
                           None))
    checks.dev_sync(dev)
    return {"g": g, "xn": xn, "wn": wn, "conv64": conv64, "y": y.cpu(), "gen": gen, "dims": (B, Ho, Wo, Cout)}


def _pad_c(x, ldc):
    """[..., C] -> [..., ldc] with zeros behind the C channels (h2 rows hold whole 32-channel groups)"""
    return F.pad(x, (0, ldc - x.shape[-1]))


def check_op_variant(lib, dev, ops, with_res, relu, log=None):
    B, Ho, Wo, Cout = ops["dims"]
    gen = ops["gen"]
    sc = torch.rand(Cout, generator=gen) * 1.5 + 0.5  # [0.5, 2]
    sh = torch.rand(Cout, generator=gen) * 2.0 - 1.0  # [-1, 1]
    res = torch.randn(B, Ho, Wo, Cout, generator=gen) if with_res else None
    ldc = (Cout + 31) // 32 * 32  # h2 rows of `out` and `res`: whole 32-channel groups
    res_h2 = to_h2(_pad_c(res, ldc)).to(dev) if with_res else None
    rv = from_h2(to_h2(_pad_c(res, ldc)))[..., :Cout] if with_res else None  # the fp32 value the residual tensor holds
    coef = torch.cat([sc, sh]).to(dev)
    out = torch.full((B, Ho, Wo, 2 * ldc), SENTINEL, dtype=torch.float16, device=dev)
    lib.check(lib.op_conv_bn_eval(H2, C.byref(ops["g"]), K(ops["xn"]), K(ops["wn"]), K(coef), K(res_h2), int(relu), K(out), ldc,
                                  K(checks.zero_page(dev)), None))
    checks.dev_sync(dev)
    raw = out.cpu()
    # 3. poison: every element written, the lo halves included -- and nothing behind the N channels of a row
    halves = raw.reshape(B, Ho, Wo, ldc // 32, 2, 32)
    ch = (torch.arange(ldc // 32).view(-1, 1, 1) * 32 + torch.arange(32).view(1, 1, -1)).expand(ldc // 32, 2, 32)
    written = (ch < Cout).expand_as(halves)
    assert not (halves[written] == SENTINEL).any().item(), "unwritten halves: %d" % int((halves[written] == SENTINEL).sum())
    assert (halves[~written] == SENTINEL).all().item(), "halves written behind channel %d" % Cout
    o = from_h2(torch.where(written, halves, torch.zeros_like(halves)).reshape(raw.shape))[..., :Cout]
    # 1. against fp64
    ref = ops["conv64"] * sc.double() + sh.double()
    if with_res:
        ref = ref + rv.double()
    if relu:
        ref = ref.clamp_min(0.0)
    err = (o.double() - ref).abs().max().item()
    tol = checks.OUT_TOL[H2] * ref.abs().max().item() + 1e-6
    # 2. against the unfused device convolution, in fp32 on the host: one fp32 rounding a fused multiply-add may or may not take,
    #    plus the h2 split's 2^-21
    y = ops["y"]
    ysc = y * sc
    v = ysc + sh
    bound = 2.0 ** -20 * (ysc.abs() + sh.abs()) + 2.0 ** -24
    if with_res:
        v = v + rv
        bound = bound + 2.0 ** -20 * rv.abs()
    pre = v
    if relu:
        v = v.clamp_min(0.0)
    d = (o - v).abs()
    worst = (d / bound).max().item()
    if log is not None:
        log("res=%d relu=%d  fp64 err %.3e (tol %.3e)  vs unfused: worst |d| / bound %.3f" % (with_res, relu, err, tol, worst))
    assert err <= tol, (err, tol)
    assert (d <= bound).all().item(), worst
    if relu:
        assert (o[pre < -bound] == 0).all().item()


def check_op(lib, dev, shape, variants=((False, False), (False, True), (True, False), (True, True)), seed=0, log=None):
    checks._fresh()
    ops = conv_operands(lib, dev, shape, seed)
    if log is not None:
        log("shape %s" % (shape,))
    for with_res, relu in variants:
        check_op_variant(lib, dev, ops, with_res, relu, log)


def check_op_refusals(lib, dev):
    checks._fresh()
    shape = (1, 4, 4, 32, 32, 1, 1, 0)
    g, Ho, Wo = checks.fwd_geom(*shape)
    x = to_h2(torch.zeros(1, 4, 4, 32)).to(dev)
    w = to_h2(torch.zeros(32, 1, 1, 32)).to(dev)
    coef = torch.zeros(64, device=dev)
    out = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device=dev)
    zp = checks.zero_page(dev)

    def call(dtype=H2, geom=g, coef_=coef, ldc=32):
        return lib.op_conv_bn_eval(dtype, C.byref(geom), K(x), K(w), K(coef_), None, 0, K(out), ldc, K(zp), None)

    assert call() == 0
    checks.dev_sync(dev)
    for dtype in (0, 1, 2, 5):
        assert call(dtype=dtype) != 0 and "dtype" in lib.last_error().decode()
    assert call(coef_=None) != 0 and "coef" in lib.last_error().decode()
    g16, _, _ = checks.fwd_geom(1, 4, 4, 16, 32, 1, 1, 0)  # C % 32 != 0
    assert call(geom=g16) != 0 and "C % 32" in lib.last_error().decode()
    g4, _, _ = checks.fwd_geom(1, 4, 4, 32, 36, 1, 1, 0)  # N % 8 != 0
    assert call(geom=g4, ldc=64) != 0 and "N % 8" in lib.last_error().decode()


# ---- plan level ----------------------------------------------------------------------------------------------------------------------
DEBUG_BLOCKS = (0, 3, 4, 15)  # layer1's first block, layer2's down block (the only one here with a projection) and the one after it, the last


def _plan(eng):
    (p,) = eng.plans.values()
    return p


def _acts(eng):
    """a1 / out (and zd of the down block) of the debug blocks after the last pass, as host tensors"""
    p = _plan(eng)
    checks.dev_sync(eng.device)
    got = {}
    for b in DEBUG_BLOCKS:
        for t in ("a1", "out"):
            got["b%d.%s" % (b, t)] = eng.debug_tensor(p, "b%d.%s" % (b, t)).cpu().clone()
    got["b3.zd"] = eng.debug_tensor(p, "b3.zd").cpu().clone()
    return got


def _model(lib, dev, dtype_name, mapnet):
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    _, net = checks.build_pair(lib, dev)
    return net if mapnet else net.mapnet


def _engine(net):
    from geomapnet_amd.posenet import engine_of
    return engine_of(net)


Y_POISON = 12345.0  # written into raw conv outputs ahead of a fused pass, which must leave them alone
ULPS = 8 * 2.0 ** -23  # "a few fp32 ulps of the pose scale": the bound where a host build does not give bit equality


def _close(a, b):
    return (a - b).abs().max().item() <= ULPS * max(1.0, b.abs().max().item())


def check_plan_bit_equal(lib, dev, dtype_name, mapnet, H, W, require=True):
    """eval() forward, set_eval_fused(True), forward, set_eval_fused(False), forward: poses and block activations equal bit for bit.
    The fused pass must not write the raw conv outputs (poisoned ahead of it: this is what tells a fused pass from a quiet unfused
    one); the unfused pass after it writes them again and reproduces the first.
    require=False (the emulator build, whose host compiler decides by itself which multiply-adds it contracts): the pass itself
    decides -- where the poses come out equal, every activation must be equal too; where they do not, the poses must agree to a few
    fp32 ulps of the pose scale.  Returns the largest pose difference."""
    checks._fresh()
    net = _model(lib, dev, dtype_name, mapnet)
    net.eval()
    if mapnet:
        x, _ = oracle.make_batch("mapnet", 1, H, W, seed=11)
    else:
        x, _ = oracle.make_batch("posenet", 3, H, W, seed=11)
    x = x.to(dev)
    eng = _engine(net)
    raw_names = ("b0.y1", "b0.y2", "b3.yd", "b3.y1", "b15.y2")
    runs = []
    for i, fused in enumerate((False, True, False)):
        net.set_eval_fused(fused)
        if fused:  # (debug_tensor gives a VIEW of an fp32 tensor of the work arena)
            for n in raw_names:
                eng.debug_tensor(_plan(eng), n).fill_(Y_POISON)
            checks.dev_sync(dev)
        with torch.no_grad():
            poses = net(x).cpu().clone()
        checks.dev_sync(dev)
        for n in raw_names:
            y = eng.debug_tensor(_plan(eng), n)
            if fused:
                assert bool((y == Y_POISON).all()), "the fused pass wrote %s" % n
            else:
                assert not bool((y == Y_POISON).any()) and bool(torch.isfinite(y).all()), "the unfused pass left %s unwritten" % n
        runs.append((poses, _acts(eng)))
    assert len(eng.plans) == 1
    assert torch.isfinite(runs[1][0]).all()
    assert torch.equal(runs[0][0], runs[2][0]) and all(torch.equal(runs[0][1][k], runs[2][1][k]) for k in runs[0][1])
    diff = (runs[0][0] - runs[1][0]).abs().max().item()
    if require or torch.equal(runs[0][0], runs[1][0]):
        assert torch.equal(runs[0][0], runs[1][0]), diff
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], runs[1][1][k]), (k, (runs[0][1][k] - runs[1][1][k]).abs().max().item())
    else:
        assert _close(runs[1][0], runs[0][0]), diff
    return diff


def check_eval_forward_fused(lib, dev, dtype_name="fp16x2m", B=3, H=64, W=85, atol=1e-3):
    """checks.check_eval_forward's comparison against the oracle, at its gate, with the switch on"""
    checks._fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    onet, net = checks.build_pair(lib, dev)
    onet, net = onet.mapnet, net.mapnet
    x, _ = oracle.make_batch("posenet", B, H, W, seed=11)
    onet.eval()
    net.eval()
    net.set_eval_fused(True)
    with torch.no_grad():
        ref = onet(x)
    out = net(x.to(dev))
    assert _plan(_engine(net)).get("eval_fused") is True
    err = (out.cpu() - ref).abs().max().item()
    assert err <= atol * max(1.0, ref.abs().max().item()), err


def _train_parts(lib, net):
    import geomapnet_amd as G
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam",
                      base_lr=1e-4, weight_decay=5e-4)
    return c, opt


def check_coefficients_never_stale(lib, dev, dtype_name="fp16x2m", N=1, T=3, H=64, W=85, require=True):
    """fused forward, one training step, fused forward = the unfused forward of the updated model; the same after load_state_dict of
    a state whose running statistics were perturbed.  require=False (the emulator): equality where the host build gives it -- the
    first pair decides -- else agreement to a few fp32 ulps of the pose scale"""
    checks._fresh()
    import geomapnet_amd as G
    net = _model(lib, dev, dtype_name, True)
    c, opt = _train_parts(lib, net)
    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    x, t = x.to(dev), t.to(dev)
    cuda = torch.device(dev).type == "cuda"

    def both():
        net.eval()
        out = []
        for fused in (True, False):
            net.set_eval_fused(fused)
            with torch.no_grad():
                out.append(net(x).cpu().clone())
        net.set_eval_fused(True)
        return out

    f0, u0 = both()
    net.train()
    G.step_feedfwd(x, net, cuda, t, c, opt, True, 0.0)
    f1, u1 = both()
    assert not torch.equal(u0, u1), "the training step must change the poses"
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = sd[k] + 0.05
        elif k.endswith("running_var"):
            sd[k] = sd[k] * 1.5
    net.load_state_dict(sd)
    f2, u2 = both()
    assert not torch.equal(u1, u2), "the perturbed statistics must change the poses"
    diffs = [(a - b).abs().max().item() for a, b in ((f0, u0), (f1, u1), (f2, u2))]
    if require or torch.equal(f0, u0):  # (require=False, the emulator: the first pair says whether the host build gives equality)
        assert torch.equal(f0, u0) and torch.equal(f1, u1) and torch.equal(f2, u2), diffs
    else:
        assert _close(f0, u0) and _close(f1, u1) and _close(f2, u2), diffs
    return diffs


def check_training_state_untouched(lib, dev, dtype_name="fp16x2m", N=2, T=3, H=64, W=85):
    """(MN_DETERMINISTIC=1 set by the caller) train step -> fused eval forward -> train step gives the bits of train step -> unfused
    eval forward -> train step: both losses, the final parameters, the running statistics and num_batches_tracked (the buffers), and
    the dropout and jitter pass counts.  The model drops (p = 0.5) and jitters its uint8 input, so a pass count that moved shows as
    another dropout mask / other jitter draws in the last step, besides the counts the host keeps."""
    checks._fresh()
    import geomapnet_amd as G
    import resize_checks as RC
    G.set_compute_dtype(dtype_name)
    x = RC.frames(N * T, H, W, seed=5).view(N, T, H, W, 3).to(dev)
    _, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    cuda = torch.device(dev).type == "cuda"
    runs = []
    for fused in (True, False):
        torch.manual_seed(7)
        net = G.MapNet(G.PoseNet(G.resnet34(_binding=lib), droprate=0.5, pretrained=False, dropout_active=True, dropout_seed=1234,
                                 _binding=lib))
        if cuda:
            net.cuda()
        net.set_input_u8(RC.MEAN, RC.STD)
        net.set_color_jitter(0.4, 0.4, 0.4, 0.1, seed=3)
        c, opt = _train_parts(lib, net)
        eng = _engine(net)
        net.train()
        l0, _ = G.step_feedfwd(x, net, cuda, t.to(dev), c, opt, True, 0.0)
        net.eval()
        net.set_eval_fused(fused)
        with torch.no_grad():
            poses = net(x).cpu().clone()
        net.train()
        l1, _ = G.step_feedfwd(x, net, cuda, t.to(dev), c, opt, True, 0.0)
        checks.dev_sync(dev)
        (p,) = [q for q in eng.plans.values() if q["cfg"].mode == 1]  # the training plan (MN_MODE_MAPNET); eval runs a PoseNet plan
        runs.append({"l0": float(l0), "l1": float(l1), "poses": poses, "params": eng.params.cpu().clone(),
                     "buffers": eng.buffers.cpu().clone(), "step": eng.effective_step(), "jitter_calls": eng.jitter_calls,
                     "plan_jitter_calls": p.get("jitter_calls"), "dropmask": eng.dropout_mask(p).cpu().clone(),
                     "draws": eng.color_jitter_draws(p)})
    a, b = runs
    for k in a:
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, k
    assert a["step"] == 2 and a["jitter_calls"] == 3 and (a["dropmask"] == 0).any()


def check_with_input_pipeline(lib, dev, dtype_name="fp16x2m"):
    """uint8 input, set_input_resize, indexed frames (IndexedFrames over a resident store) and a fused eval forward give the bits of the
    unfused one, at the smallest plan shape tests/resident_checks.py uses"""
    checks._fresh()
    import resident_checks as RS
    from geomapnet_amd.resident import IndexedFrames
    net = RS._net(lib, dev, dtype_name)
    net.set_input_resize((RS.PLAN_H, RS.PLAN_W))
    store = RS._stores(dev)["u8_src"]
    idx = torch.tensor(RS.PLAN_INDEX, dtype=torch.int64)
    out = []
    for fused in (False, True):
        net.set_eval_fused(fused)
        with torch.no_grad():
            out.append(net(IndexedFrames(store, idx)).cpu().clone())
    assert tuple(out[0].shape) == (1, 3, 6) and torch.isfinite(out[1]).all()
    assert torch.equal(out[0], out[1]), (out[0] - out[1]).abs().max().item()


def check_refusals(lib, dev):
    """set_eval_fused(True) on fp32, fp32x3 and fp16 models raises with the dtype named -- from the model before it has a plan, and
    from the library for a plan that exists"""
    checks._fresh()
    import geomapnet_amd as G
    from geomapnet_amd._binding import MapNetHipError
    for name in ("fp32", "fp32x3", "fp16"):
        net = _model(lib, dev, name, True)
        net.eval()
        try:
            net.set_eval_fused(True)
            raise AssertionError("%s must be refused" % name)
        except MapNetHipError as e:
            assert name in str(e) and "h2" in str(e), str(e)
        assert _engine(net).eval_fused is False
    # the library's own refusal, through a plan of an fp32 model
    net = _model(lib, dev, "fp32", False)
    net.eval()
    with torch.no_grad():
        net(torch.randn(1, 3, 32, 40).to(dev))
    p = _plan(_engine(net))
    assert lib.set_eval_fused(p["handle"], 1) != 0
    msg = lib.last_error().decode()
    assert "fp32" in msg and "mn_set_eval_fused" in msg, msg
    assert lib.set_eval_fused(p["handle"], 0) == 0
    # off is accepted everywhere; on is accepted by the h2 modes
    net.set_eval_fused(False)
    G.set_compute_dtype("fp16x2m")
    m = _model(lib, dev, "fp16x2m", True)
    m.set_eval_fused(True)
    assert _engine(m).eval_fused is True


def check_command_lines(lib, tmp_path, H=64, W=85):
    """scripts/eval.py --fused_eval on a checkpoint from scripts/train.py (--fused_eval: its validation passes) on synthetic frames
    prints the four error figures of the run without the flag; the predicted poses are equal bit for bit"""
    import configparser
    import os
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import eval as eval_script
    import train as train_script
    s = configparser.ConfigParser()
    s.read(os.path.join(root, "scripts", "configs", "synthetic_mapnet.ini"))
    s["training"].update(n_epochs="1", batch_size="2", snapshot="1", val_freq="1", do_val="yes")
    s["hyperparameters"]["skip"] = "1"
    cfg = str(tmp_path / "synthetic_mapnet.ini")
    with open(cfg, "w") as f:
        s.write(f)
    size = ["--synthetic_length", "4", "--height", str(H), "--width", str(W)]
    targs = train_script.build_parser().parse_args(
        ["--model", "mapnet", "--config_file", cfg, "--dtype", "fp16x2m", "--synthetic_val_length", "2", "--logdir",
         str(tmp_path / "logs"), "--num_workers", "0", "--fused_eval"] + size)
    lines = []
    tr = train_script.run(targs, _binding=lib, log=lines.append)
    assert os.path.isfile(tr.final_checkpoint)
    got = []
    for extra in ([], ["--fused_eval"]):
        eargs = eval_script.build_parser().parse_args(
            ["--model", "mapnet", "--config_file", cfg, "--weights", tr.final_checkpoint, "--dtype", "fp16x2m", "--val"] + size + extra)
        out = []
        summary, pred, _ = eval_script.run(eargs, _binding=lib, log=out.append)
        got.append(([ln for ln in out if ln.startswith("Error in")], pred))
    assert got[0][0] and got[0][0] == got[1][0], got
    assert np.isfinite(got[1][1]).all() and np.array_equal(got[0][1], got[1][1])
