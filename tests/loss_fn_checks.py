"""Backend-agnostic checks of the criteria's loss functions (csrc/criterion.h criterion_kernel<true>, mn_op_criterion_fn,
mn_set_loss_fn): each takes a Binding (`lib`) and a torch device, so the CPU suite runs them on the SIMT-emulator build and the GPU
suite on libmapnet_hip.so.  The reference side is tests/loss_fn_ref.py in float64 under autograd."""
import os

import numpy as np
import torch
from torch import nn

import checks
import loss_fn_ref as REF
import oracle
from checks import K, f32

L1, MSE, SMOOTH_L1, HUBER, QUATERNION = range(5)  # enum mn_loss_kind
T_KINDS = (L1, MSE, SMOOTH_L1, HUBER)
Q_KINDS = (L1, MSE, SMOOTH_L1, HUBER, QUATERNION)
S4 = [0.3, -2.5, 0.7, -3.5]  # the log-weights of checks.check_criterion_vs_oracle


def module(kind, param):
    return {L1: nn.L1Loss, MSE: nn.MSELoss, SMOOTH_L1: lambda: nn.SmoothL1Loss(beta=param), HUBER: lambda: nn.HuberLoss(delta=param),
            QUATERNION: REF.QuaternionLoss}[kind]()


def run(lib, dev, mode, pred, targ, s4, fn, grads=True):
    """mn_op_criterion_fn (fn = (t_kind, t_param, q_kind, q_param)), or mn_op_criterion for fn None -> loss [1], dpred, ds [4] on the
    CPU (dpred / ds None when forward-only)"""
    pred, targ = pred.contiguous().to(dev), targ.contiguous().to(dev)
    n = pred.shape[0]
    T = 1 if mode == 0 else (pred.shape[1] if mode == 1 else pred.shape[1] // 2)
    loss = torch.full((1,), 7.0, device=dev)
    dp = torch.full_like(pred, 7.0) if grads else None  # poison: every element must be written
    ds = torch.zeros(4, device=dev) if grads else None
    s = torch.tensor(s4, dtype=torch.float32, device=dev)
    if fn is None:
        lib.check(lib.op_criterion(mode, n, T, K(pred), K(targ), K(s), K(loss), K(dp), K(ds), None, f32(1.0), None))
    else:
        lib.check(lib.op_criterion_fn(mode, n, T, K(pred), K(targ), K(s), K(loss), K(dp), K(ds), None, f32(1.0), fn[0], f32(fn[1]),
                                      fn[2], f32(fn[3]), None))
    checks.dev_sync(dev)
    return loss.cpu(), (dp.cpu() if grads else None), (ds.cpu() if grads else None)


def inputs(mode, N, T, seed=0):
    """the seeded poses of checks.check_criterion_vs_oracle: translations ~ N(0,1), log-quaternions as oracle.make_batch, predictions
    0.3 N(0,1) around them"""
    name = REF.MODES[mode]
    om = {"posenet": "posenet", "mapnet": "mapnet", "online": "mapnet++", "gps": "mapnet++"}[name]
    _, targ = oracle.make_batch(om, N, 1, 1, t=T, seed=100 + seed, gps_mode=(mode == 3))
    gen = torch.Generator().manual_seed(seed)
    shape = (N, 6) if mode == 0 else (N, T, 6) if mode == 1 else (N, 2 * T, 6)
    lead = targ if mode <= 1 else torch.cat((targ[:, :T], oracle.make_batch("mapnet", N, 1, 1, t=T, seed=7 + seed)[1]), 1)
    return (lead + 0.3 * torch.randn(*shape, generator=gen)).contiguous(), targ.contiguous()


def split_param(d):
    """a beta / delta (an fp32 value) between the two middle |differences|: both pieces of SmoothL1 / Huber are populated"""
    a = d.abs().sort().values
    k = a.numel() // 2
    return float(np.float32(0.5 * (a[k - 1].item() + a[k].item()))) if a.numel() > 1 else float(np.float32(a[0].item() * 2))


def reference(mode, pred, targ, s4, t_mod, q_mod):
    crit = REF.make(mode, t_mod, q_mod, s4).double()
    p64 = pred.double().requires_grad_(True)
    want = crit(p64, targ.double())
    want.backward()
    names = ("sax", "saq") if mode == 0 else ("sax", "saq", "srx") if mode == 3 else ("sax", "saq", "srx", "srq")
    return want.item(), p64.grad, [getattr(crit, n).grad.item() for n in names]


def compare(got, want, what):
    """the tolerances of checks.check_criterion_vs_oracle: loss 2e-5, dpred rtol 3e-4 / atol 3e-6, d s 2e-4"""
    (loss, dp, ds), (wl, wdp, wds) = got, want
    print("%s: loss %.7g (reference %.7g)" % (what, loss.item(), wl))
    assert abs(loss.item() - wl) <= 2e-5 * max(1.0, abs(wl)), (what, loss.item(), wl)
    if dp is None:
        return
    np.testing.assert_allclose(dp.numpy(), wdp.float().numpy(), rtol=3e-4, atol=3e-6, err_msg=str(what))
    for i, w in enumerate(wds):
        assert abs(ds[i].item() - w) <= 2e-4 * max(1.0, abs(w)), (what, i, ds[i].item(), w)
    assert all(ds[i].item() == 0.0 for i in range(len(wds), 4)), (what, ds)  # the terms the mode does not have stay untouched


def check_pairs(lib, dev, mode, N, T, seed=0):
    """every (t kind, q kind) pair on one shape, with gradients and forward-only, against the float64 restatement; beta / delta split
    the reference differences of the case in the middle, and the test requires both pieces to hold >= 20 % of the elements"""
    checks._fresh()
    pred, targ = inputs(mode, N, T, seed)
    dt, dq = REF.differences(mode, pred, targ)
    prm = {False: split_param(dt), True: split_param(dq)}
    for rot, d in ((False, dt), (True, dq)):
        inner = (d.abs() < prm[rot]).double().mean().item()
        assert d.numel() < 2 or (0.2 <= inner <= 0.8), ("pieces of SmoothL1 / Huber", mode, N, T, rot, inner)
    for tk in T_KINDS:
        for qk in Q_KINDS:
            fn = (tk, prm[False] if tk in (SMOOTH_L1, HUBER) else 0.0, qk, prm[True] if qk in (SMOOTH_L1, HUBER) else 0.0)
            want = reference(mode, pred, targ, S4, module(fn[0], fn[1]), module(fn[2], fn[3]))
            what = (REF.MODES[mode], N, T, fn)
            got = run(lib, dev, mode, pred, targ, S4, fn, grads=True)
            compare(got, want, what)
            fwd = run(lib, dev, mode, pred, targ, S4, fn, grads=False)
            assert torch.equal(fwd[0], got[0]), what  # forward-only: the same loss, bit for bit


def hand_built(param, N=4, T=2, seed=5):
    """mode-1 poses whose differences are exact multiples of param / 2 in {0, +-param/2, +-param, +-2 param, 3 param} (0 and +-param in
    every window), on targets that are multiples of 1/4: every difference, and every VO difference, is exact in fp32"""
    gen = torch.Generator().manual_seed(seed)
    targ = torch.randint(-8, 9, (N, T, 6), generator=gen).float() / 4.0
    b = param if param > 0 else 0.5
    vals = torch.tensor([0.0, b, -b, 0.5 * b, -0.5 * b, 2 * b, -2 * b, 3 * b])
    d = vals[torch.randint(0, 8, (N, T, 6), generator=gen)]
    d[:, 0, 0], d[:, 0, 1], d[:, 0, 2] = 0.0, b, -b
    d[:, 1, 3], d[:, 1, 4], d[:, 1, 5] = 0.0, -b, b
    pred = targ + d
    assert torch.equal(pred - targ, d)
    return pred.contiguous(), targ.contiguous()


def check_hand_built(lib, dev, kind):
    """d = 0 and d = +-param exactly (and values on both sides) for a piecewise kind as t and q loss, at the operator tolerances;
    SmoothL1 with beta = 0 is the L1 result bit for bit"""
    checks._fresh()
    for param in (0.5, 0.75):
        pred, targ = hand_built(param)
        fn = (kind, param, kind, param)
        want = reference(1, pred, targ, S4, module(kind, param), module(kind, param))
        compare(run(lib, dev, 1, pred, targ, S4, fn), want, ("hand-built", fn))
    if kind == SMOOTH_L1:
        pred, targ = hand_built(0.0)
        got = run(lib, dev, 1, pred, targ, S4, (SMOOTH_L1, 0.0, SMOOTH_L1, 0.0))
        l1 = run(lib, dev, 1, pred, targ, S4, None)
        for a, b in zip(got, l1):
            assert torch.equal(a, b)
        compare(got, reference(1, pred, targ, S4, nn.SmoothL1Loss(beta=0.0), nn.SmoothL1Loss(beta=0.0)), "hand-built beta = 0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def check_default_op_unchanged(lib, dev, golden_dir):
    """mn_op_criterion and mn_op_criterion_fn(L1, 0, L1, 0) on the golden inputs (all four modes, the NaN case included): the same
    bits in loss, dpred and ds"""
    checks._fresh()
    cases = checks.golden_cases(golden_dir)
    modes = set()
    for name, d in cases.items():
        mode = 0 if name.startswith("posenet") else 1 if name.startswith("mapnet") else 3 if name.startswith("gps") else 2
        modes.add(mode)
        s4 = [float(d.get("s_" + n, 0.0)) for n in ("sax", "saq", "srx", "srq")]
        pred, targ = torch.from_numpy(d["pred"]), torch.from_numpy(d["targ"])
        for grads in (True, False):
            a = run(lib, dev, mode, pred, targ, s4, None, grads)
            b = run(lib, dev, mode, pred, targ, s4, (L1, 0.0, L1, 0.0), grads)
            for x, y in zip(a, b):
                assert (x is None and y is None) or torch.equal(_bits(x), _bits(y)), name
    assert modes == {0, 1, 2, 3}


def _model(lib, dev, crit_kw):
    import geomapnet_amd as G
    onet, net = checks.build_pair(lib, dev)
    c = G.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, _binding=lib, **crit_kw)
    opt = G.Optimizer([{"params": net.parameters()}, {"params": [c.sax, c.saq]}, {"params": [c.srx, c.srq]}], "adam", base_lr=1e-4,
                      weight_decay=5e-4)
    net.train()
    return onet, net, c, opt


def check_default_plan_unchanged(lib, dev, dtype_name="fp32", N=1, H=32, W=40):
    """(MN_DETERMINISTIC=1 set by the caller before the library read its knobs) two training steps on a plan mn_set_loss_fn never
    touched, and on a twin whose plan was set to MSE / Huber and then to L1 / L1 before its first step: bit-equal losses and poses"""
    checks._fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    cuda = torch.device(dev).type == "cuda"
    runs = []
    for touch in (False, True):
        _, net, c, opt = _model(lib, dev, {})
        eng = net.mapnet._engine
        if touch:
            p = eng.plan(1, N, x.shape[1], H, W)
            lib.check(lib.set_loss_fn(p["handle"], MSE, f32(0.0), HUBER, f32(0.25)))
            lib.check(lib.set_loss_fn(p["handle"], L1, f32(0.0), L1, f32(0.0)))
        out = []
        for _ in range(2):
            l, poses = G.step_feedfwd(x.to(dev), net, cuda, t.to(dev), c, opt, True, 0.0)
            out.append((float(l), poses.cpu().clone()))
        assert "loss_fn" not in eng.plan(1, N, x.shape[1], H, W)  # an L1 criterion never makes the engine call mn_set_loss_fn
        runs.append(out)
    for (la, pa), (lb, pb) in zip(*runs):
        assert la == lb and torch.equal(pa, pb)
    assert runs[0][0][0] != runs[0][1][0]  # (the second step saw updated weights)


def check_fused_step(lib, dev, dtype_name, N=2, H=64, W=85, beta=0.3):
    """one training step of MapNet with MSELoss (translation) and SmoothL1Loss (rotation), learned beta and gamma, against the oracle
    network under the restated criterion at checks.check_train_step's bars for L1 (loss 1e-4, poses 1e-3, every parameter gradient
    2e-2 relative L2, criterion-scalar gradients 1e-3).  Then the losses alternate on the one model: an L1 validation step without an
    optimiser (= the stand-alone MapNetCriterion() on the returned poses), the plan's own loss entry (mn_loss) switched to L1 / L1 by
    the engine (= the stand-alone L1 criterion with the model's log-weights), and a third step that switches the plan back to
    MSE / SmoothL1 and is compared with the oracle's second step at check_train_step's bars for later steps."""
    checks._fresh()
    import geomapnet_amd as G
    G.set_compute_dtype(dtype_name)
    fns = lambda: dict(t_loss_fn=nn.MSELoss(), q_loss_fn=nn.SmoothL1Loss(beta=beta))  # noqa: E731
    onet, net, c, opt = _model(lib, dev, fns())
    oc = REF.MapNetCriterion(sax=0.0, saq=-3.0, srx=0.0, srq=-3.0, learn_beta=True, learn_gamma=True, **fns())
    oopt = oracle.Optimizer([{"params": onet.parameters()}, {"params": [oc.sax, oc.saq]}, {"params": [oc.srx, oc.srq]}], "adam",
                            base_lr=1e-4, weight_decay=5e-4)
    onet.train()
    x, t = oracle.make_batch("mapnet", N, H, W, seed=7)
    cuda = torch.device(dev).type == "cuda"
    xd, td = x.to(dev), t.to(dev)

    lo, po = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True, 0.0)
    l, p = G.step_feedfwd(xd, net, cuda, td, c, opt, True, 0.0)
    pose_err = (p.cpu() - po.detach()).abs().max().item()
    inner = ((po.detach()[..., 3:] - t[..., 3:]).abs() < beta).float().mean().item()
    print("fused step %s: loss %.7g (oracle %.7g), max pose err %.2e; %.0f %% of the absolute rotation differences on the quadratic "
          "piece" % (dtype_name, l, lo, pose_err, 100 * inner))
    assert abs(l - lo) <= 1e-4 * max(1.0, abs(lo)), (l, lo)
    assert pose_err <= 1e-3, pose_err
    eng = net.mapnet._engine
    plan = eng.plan(1, N, x.shape[1], H, W)
    assert plan["loss_fn"] == (MSE, 0.0, SMOOTH_L1, beta)
    og = dict(onet.named_parameters())
    worst = 0.0
    for e in eng.entries:
        if e.is_buffer:
            continue
        g = checks._view(eng.grads(), e).cpu().double()
        r = og["mapnet." + e.name.decode()].grad.double()
        if r.norm() >= 1e-8:
            worst = max(worst, ((g - r).norm() / r.norm()).item())
    print("fused step %s: worst parameter gradient relative L2 %.3e" % (dtype_name, worst))
    assert worst <= 2e-2, worst
    cg = eng.grads()[-4:].cpu().numpy()
    for i, nm in enumerate(("sax", "saq", "srx", "srq")):
        ref = getattr(oc, nm).grad.item()
        assert abs(cg[i] - ref) <= 1e-3 * max(1.0, abs(ref)), (nm, cg[i], ref)

    # validation with another criterion (L1, no learned weights) on the same model, no optimiser: common/train.py:343-351
    val = G.MapNetCriterion(_binding=lib)
    vl, vout = G.step_feedfwd(xd, net, cuda, td, val, None, False)
    assert vl == G.MapNetCriterion(_binding=lib).forward(vout, td).item()
    assert np.isfinite(vl) and vl != l
    # the plan's own loss entry: the engine switches the plan to L1 / L1 (it tells the library: the setting differs) ...
    eng.set_loss_fn(plan, val.loss_fn)
    assert plan["loss_fn"] == (L1, 0.0, L1, 0.0)
    out = torch.zeros(1, device=dev)
    poses = vout.reshape(-1, 6).contiguous()
    lib.check(lib.loss(plan["handle"], K(poses), K(td.contiguous()), K(out), None))
    checks.dev_sync(dev)
    s_now = [float(v) for v in eng.crit_slice().cpu()]
    same = G.MapNetCriterion(sax=s_now[0], saq=s_now[1], srx=s_now[2], srq=s_now[3], _binding=lib)
    assert out.item() == same.forward(vout, td).item()
    # ... and the next training step switches it back
    lo2, po2 = oracle.step_feedfwd(x, onet, False, t, oc, oopt, True, 0.0)
    l2, p2 = G.step_feedfwd(xd, net, cuda, td, c, opt, True, 0.0)
    assert plan["loss_fn"] == (MSE, 0.0, SMOOTH_L1, beta)
    print("fused step %s, third call: loss %.7g (oracle's second step %.7g)" % (dtype_name, l2, lo2))
    assert abs(l2 - lo2) <= 5e-3 * max(1.0, abs(lo2)), (l2, lo2)  # (check_train_step's bars for steps after the first)
    assert (p2.cpu() - po2.detach()).abs().max().item() <= 2e-2 * max(1.0, po2.abs().max().item())


def check_facade(lib, dev):
    """accepted classes -> kinds and parameters; the attributes; everything else NotImplementedError naming what is supported; the C
    entries refuse the same with a message"""
    checks._fresh()
    import geomapnet_amd as G
    from geomapnet_amd import criterion as GC
    assert (GC.LOSS_L1, GC.LOSS_MSE, GC.LOSS_SMOOTH_L1, GC.LOSS_HUBER, GC.LOSS_QUATERNION) == (L1, MSE, SMOOTH_L1, HUBER, QUATERNION)
    for cls in (G.PoseNetCriterion, G.MapNetCriterion, G.MapNetOnlineCriterion):
        c = cls(_binding=lib)
        assert isinstance(c.t_loss_fn, nn.L1Loss) and isinstance(c.q_loss_fn, nn.L1Loss) and c.loss_fn == (L1, 0.0, L1, 0.0)
        t_fn, q_fn = nn.SmoothL1Loss(beta=0.25), nn.HuberLoss(delta=1.5)
        c = cls(t_fn, q_fn, _binding=lib)
        assert c.t_loss_fn is t_fn and c.q_loss_fn is q_fn and c.loss_fn == (SMOOTH_L1, 0.25, HUBER, 1.5)
        c = cls(t_loss_fn=nn.MSELoss(), q_loss_fn=G.QuaternionLoss(), _binding=lib)
        assert c.loss_fn == (MSE, 0.0, QUATERNION, 0.0)
        assert set(c.state_dict()) <= {"sax", "saq", "srx", "srq"}  # the loss modules add nothing to a checkpoint
        for bad in (dict(t_loss_fn=nn.L1Loss(reduction="sum")), dict(q_loss_fn=nn.MSELoss(reduction="none")),
                    dict(t_loss_fn=G.QuaternionLoss()), dict(q_loss_fn=nn.CrossEntropyLoss()), dict(t_loss_fn=lambda a, b: (a - b).sum()),
                    dict(q_loss_fn=nn.SmoothL1Loss(beta=-1.0))):
            try:
                cls(_binding=lib, **bad)
                raise AssertionError("%r must raise" % (bad,))
            except NotImplementedError as e:
                assert "nn.HuberLoss" in str(e) and "QuaternionLoss" in str(e), str(e)
    # QuaternionLoss on its own is the reference's formula
    a, b = torch.randn(5, 3, dtype=torch.float64), torch.randn(5, 3, dtype=torch.float64)
    assert torch.equal(G.QuaternionLoss()(a, b), REF.QuaternionLoss()(a, b))
    # the stand-alone forward passes the kinds down
    pred, targ = inputs(1, 5, 3)
    c = G.MapNetCriterion(nn.MSELoss(), G.QuaternionLoss(), sax=S4[0], saq=S4[1], srx=S4[2], srq=S4[3], _binding=lib)
    want = reference(1, pred, targ, S4, nn.MSELoss(), REF.QuaternionLoss())[0]
    got = c(pred.to(dev), targ.to(dev)).item()
    assert abs(got - want) <= 2e-5 * max(1.0, abs(want))
    # the C entries
    for fn, word in (((QUATERNION, 0.0, L1, 0.0), "rotation"), ((L1, -0.5, L1, 0.0), ">= 0"), ((L1, 0.0, HUBER, -1.0), ">= 0"),
                     ((5, 0.0, L1, 0.0), "unknown"), ((L1, 0.0, -1, 0.0), "unknown"), ((L1, 0.0, 5, 0.0), "unknown")):
        loss = torch.zeros(1, device=dev)
        s = torch.zeros(4, device=dev)
        rc = lib.op_criterion_fn(1, 5, 3, K(pred.to(dev)), K(targ.to(dev)), K(s), K(loss), None, None, None, f32(1.0), fn[0], f32(fn[1]),
                                 fn[2], f32(fn[3]), None)
        assert rc != 0 and word in lib.last_error().decode(), (fn, lib.last_error())
    G.set_compute_dtype("fp32")
    _, net = checks.build_pair(lib, dev)
    p = net.mapnet._engine.plan(1, 1, 2, 32, 40)
    for fn, word in (((QUATERNION, 0.0, L1, 0.0), "rotation"), ((MSE, -1.0, L1, 0.0), ">= 0"), ((7, 0.0, L1, 0.0), "unknown")):
        assert lib.set_loss_fn(p["handle"], fn[0], f32(fn[1]), fn[2], f32(fn[3])) != 0
        assert "mn_set_loss_fn" in lib.last_error().decode() and word in lib.last_error().decode()
    assert lib.set_loss_fn(p["handle"], HUBER, f32(1.0), QUATERNION, f32(0.0)) == 0
