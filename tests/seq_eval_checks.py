"""Backend-agnostic checks of sequence evaluation (csrc/seq_eval.h mn_seq_windows, pgo.optimize_windows_dev, evaluate.predict_frames /
evaluate_sequence): each takes a Binding (`lib`) and a torch device, so the CPU suite runs them on the SIMT-emulator build and the GPU
suite on libmapnet_hip.so.  References: the host functions the kernel restates (evaluate.to_pose7, data.calc_vos_safe /
calc_vos_safe_fc), the window loop `evaluate.evaluate`, and the oracle's forward pass."""
import numpy as np
import torch

import checks
import input_grad_checks as IG
from geomapnet_amd import evaluate as E
from geomapnet_amd import pgo as P
from geomapnet_amd._binding import MapNetHipError, ptr
from geomapnet_amd.data import MF, SyntheticFrames, calc_vos_safe, calc_vos_safe_fc
from geomapnet_amd.resident import ResidentFrames

MEAN, STD = IG.MEAN, IG.STD
VO_ATOL = 2e-6   # checks.check_calc_vos_golden's bound on the device VO
POISON = float("nan")
SENTINEL, GUARD = 7.0, 16
L = 50
# (W, N, fc): one window of the smallest size; 300 windows are no multiple of a workgroup; N = 12 is the optimiser's limit (66 pairs)
OP_CASES = ((1, 2, False), (300, 3, False), (300, 7, True), (65, 12, True))

_ZERO = np.zeros(3), np.ones(3)  # to_pose7 without un-normalisation: qexp only


# ---- inputs: computed once, shared, left unchanged ------------------------------------------------------------------------------------
def _qexp64(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.concatenate((np.cos(n), np.sinc(n / np.pi) * v), axis=-1)


_TABLES = {}


def tables(seed=5):
    """(pose_table, vo_table) fp32 [L,6]: translations N(0,1); log-quaternions of norm <= 0.6, drawn one by one and kept only if the
    relative half-angle to every row kept so far is at least 0.2 rad -- so every pair of distinct rows has a relative half-angle in
    [0.2, 1.2] (half-angles add at most), away from arccos' ill-conditioned end in fp32"""
    if seed not in _TABLES:
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(2):
            logq = np.zeros((0, 3))
            while len(logq) < L:
                v = rng.normal(size=3)
                v *= 0.6 * rng.uniform() ** (1.0 / 3.0) / np.linalg.norm(v)
                if len(logq):
                    half = np.arccos(np.clip(np.abs(_qexp64(logq) @ _qexp64(v)), 0.0, 1.0))
                    if half.min() < 0.2:
                        continue
                logq = np.vstack((logq, v))
            q = _qexp64(logq)
            half = np.arccos(np.clip(np.abs(q @ q.T), 0.0, 1.0))[~np.eye(L, dtype=bool)]
            assert half.min() >= 0.2 and half.max() <= 1.2
            out.append(torch.from_numpy(np.hstack((rng.normal(size=(L, 3)), logq)).astype(np.float32)))
        _TABLES[seed] = tuple(out)
    return _TABLES[seed]


def windows(W, N, seed):
    """[W,N] int32: N distinct rows per window"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(L)[:N] for _ in range(W)]).astype(np.int32)


def clamped_windows():
    """the real windows of MF(steps=3, skip=2) over 9 frames: [0,0,2] ... [6,8,8]"""
    mf = MF(SyntheticFrames(9, H=8, W=8), steps=3, skip=2)
    win = np.stack([mf.get_indices(i) for i in range(len(mf))]).astype(np.int32)
    assert win[0].tolist() == [0, 0, 2] and win[-1].tolist() == [6, 8, 8] and win.shape == (9, 3)
    return win


_HOST = {}


def host_windows(pose_table, vo_table, win, fc):
    """the restatement: (poses7 [W,N,7] fp64, vo six-vectors [W,P,6] fp32, vos7 [W,P,7] fp64) from table[win]"""
    key = (pose_table.data_ptr(), vo_table.data_ptr(), win.tobytes(), win.shape, bool(fc))
    if key not in _HOST:
        idx = torch.from_numpy(win.astype(np.int64))
        W, N = win.shape
        poses7 = E.to_pose7(pose_table[idx].numpy().reshape(-1, 6), *_ZERO).reshape(W, N, 7)
        vos = (calc_vos_safe_fc if fc else calc_vos_safe)(vo_table[idx])
        vos7 = E.to_pose7(vos.numpy().reshape(-1, 6), *_ZERO).reshape(W, -1, 7)
        _HOST[key] = (pose_table, vo_table, poses7, vos.numpy(), vos7)
    return _HOST[key][2:]


# ---- mn_seq_windows -----------------------------------------------------------------------------------------------------------------
def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    buf[GUARD:GUARD + n] = POISON  # every element must be written
    return buf


def run_op(lib, dev, pose_table, vo_table, win, fc, flag_preset=7.0):
    """-> (poses7 [W,N,7], vos7 [W,P,7] or None, flag); the doubles around both outputs keep their sentinel, the inputs are unchanged"""
    W, N = win.shape
    Pn = N * (N - 1) // 2 if fc else N - 1
    pt, wn = pose_table.to(dev), torch.from_numpy(win).to(dev)
    vt = None if vo_table is None else vo_table.to(dev)
    b7 = _guarded(W * N * 7, dev)
    bv = None if vo_table is None else _guarded(W * Pn * 7, dev)
    flag = torch.full((1,), flag_preset, dtype=torch.float32, device=dev)
    lib.check(lib.seq_windows(ptr(pt), ptr(vt), ptr(wn), pose_table.shape[0], W, N, int(fc), ptr(b7[GUARD:]),
                              None if bv is None else ptr(bv[GUARD:]), ptr(flag), None))
    checks.dev_sync(dev)
    outs = []
    for buf, rows in ((b7, N), (bv, Pn)):
        if buf is None:
            outs.append(None)
            continue
        b = buf.cpu()
        assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), "the kernel wrote outside its output"
        outs.append(b[GUARD:-GUARD].view(W, rows, 7).numpy())
    assert torch.equal(pt.cpu(), pose_table) and torch.equal(wn.cpu(), torch.from_numpy(win))
    return outs[0], outs[1], flag.cpu().item()


def six_of(vos7):
    """the fp32 six-vector the device took the qexp of, recovered from its fp64 row: the translation as it stands, the rotation by
    the fp64 logarithm (well conditioned at these angles: exact to ~1e-15, far inside half an fp32 ulp) rounded to fp32"""
    q = vos7[..., 3:]
    nv = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    logq = np.where(nv > 0, np.arccos(np.clip(q[..., :1], -1.0, 1.0)) * q[..., 1:] / np.where(nv > 0, nv, 1.0), 0.0)
    return np.concatenate((vos7[..., :3], logq), axis=-1).astype(np.float32)


def check_op_case(lib, dev, W, N, fc):
    pose_table, vo_table = tables()
    win = windows(W, N, seed=100 + N)
    poses7, vos7, flag = run_op(lib, dev, pose_table, vo_table, win, fc)
    want7, want_vo, want_vos7 = host_windows(pose_table, vo_table, win, fc)
    assert flag == 0.0, "a clean call must clear the flag"
    assert np.isfinite(poses7).all() and np.isfinite(vos7).all(), "an output element was not written"
    e7 = np.abs(poses7 - want7).max()
    six = six_of(vos7)
    assert np.array_equal(six[..., :3].astype(np.float64), vos7[..., :3]), "VO translations must be fp32 values"
    e_vo = np.abs(six.astype(np.float64) - want_vo.astype(np.float64)).max()
    e_exp = np.abs(vos7 - E.to_pose7(six.reshape(-1, 6), *_ZERO).reshape(vos7.shape)).max()  # the qexp step on exact inputs
    checks._record_deviation({"check": "seq_windows", "W": W, "N": N, "fc": bool(fc), "dev": str(dev), "poses7_abs_max": float(e7),
                              "vo6_abs_max": float(e_vo), "vos7_qexp_abs_max": float(e_exp)})
    print("seq_windows (%d, %d, %s): poses7 %.2e, VO six-vectors %.2e, VO qexp %.2e" % (W, N, fc, e7, e_vo, e_exp))
    assert e7 <= checks.PGO_TOL, e7
    assert e_exp <= checks.PGO_TOL, e_exp
    assert e_vo <= VO_ATOL, e_vo
    # without a VO table: the same poses7, vos7 not touched
    only7, none, flag = run_op(lib, dev, pose_table, None, win, fc)
    assert none is None and flag == 0.0 and np.array_equal(only7, poses7)


def check_op_clamped(lib, dev):
    """windows that repeat the boundary frame: the VO of a frame with itself is exactly the identity, as on the host"""
    pose_table, vo_table = tables()
    win = clamped_windows()
    for fc in (False, True):
        poses7, vos7, flag = run_op(lib, dev, pose_table, vo_table, win, fc)
        want7, _, want_vos7 = host_windows(pose_table, vo_table, win, fc)
        pairs = [(i, j) for i in range(3) for j in range(i + 1, 3)] if fc else [(0, 1), (1, 2)]
        same = np.array([[w[i] == w[j] for (i, j) in pairs] for w in win])
        assert same.sum() == 2 and same[0, 0] and same[-1, -1]
        identity = torch.tensor([0.0, 0, 0, 1, 0, 0, 0], dtype=torch.float64)
        for row in torch.from_numpy(vos7)[torch.from_numpy(same)]:
            assert torch.equal(row, identity), row
        assert torch.equal(torch.from_numpy(vos7)[torch.from_numpy(same)], torch.from_numpy(want_vos7)[torch.from_numpy(same)])
        assert flag == 0.0 and np.abs(poses7 - want7).max() <= checks.PGO_TOL
        assert np.abs(six_of(vos7)[~same].astype(np.float64) - six_of(want_vos7)[~same]).max() <= VO_ATOL


def check_op_bounds_guard(lib, dev):
    """emulator only (never aim a bad index at a shared GPU): the flag is set, the slot reads row 0, the other windows are untouched"""
    pose_table, vo_table = tables()
    good = windows(6, 3, seed=9)
    bad = good.copy()
    bad[1, 2], bad[4, 0] = -1, L
    fixed = bad.copy()
    fixed[1, 2], fixed[4, 0] = 0, 0
    for fc in (False, True):
        p_bad, v_bad, flag = run_op(lib, dev, pose_table, vo_table, bad, fc)
        assert flag == 1.0
        p_fix, v_fix, flag = run_op(lib, dev, pose_table, vo_table, fixed, fc)
        assert flag == 0.0
        assert np.array_equal(p_bad, p_fix) and np.array_equal(v_bad, v_fix)
        p_good, v_good, _ = run_op(lib, dev, pose_table, vo_table, good, fc)
        keep = [0, 2, 3, 5]
        assert np.array_equal(p_bad[keep], p_good[keep]) and np.array_equal(v_bad[keep], v_good[keep])


def check_op_errors(lib, dev):
    pose_table, vo_table = tables()
    pt, vt = pose_table.to(dev), vo_table.to(dev)
    out = torch.zeros(13 * 78 * 7, dtype=torch.float64, device=dev)
    for N, word in ((1, "poses per window"), (13, "poses per window")):
        wn = torch.zeros(1, N, dtype=torch.int32, device=dev)
        assert lib.seq_windows(ptr(pt), ptr(vt), ptr(wn), L, 1, N, 0, ptr(out), ptr(out), None, None) != 0
        assert word in lib.last_error().decode(), lib.last_error().decode()
    wn = torch.zeros(1, 3, dtype=torch.int32, device=dev)
    for args, word in (((ptr(pt), None, ptr(wn), L, 1, 3, 0, ptr(out), ptr(out), None, None), "both or neither"),
                       ((ptr(pt), ptr(vt), ptr(wn), L, 1, 3, 0, ptr(out), None, None, None), "both or neither"),
                       ((ptr(pt), ptr(vt), ptr(wn), L, 0, 3, 0, ptr(out), ptr(out), None, None), "at least 1"),
                       ((None, ptr(vt), ptr(wn), L, 1, 3, 0, ptr(out), ptr(out), None, None), "required")):
        assert lib.seq_windows(*args) != 0
        assert word in lib.last_error().decode(), (word, lib.last_error().decode())


# ---- pgo.optimize_windows_dev --------------------------------------------------------------------------------------------------------
def check_optimize_windows_dev(lib, dev):
    """device tensors in, a device tensor out, the numbers of optimize_windows; LinAlgError as there"""
    pred, vos, _ = checks.pgo_windows(5, 4, True, seed=13)
    want = P.optimize_windows(pred, vos, fc_vos=True, srx=2.0, device=dev, binding=lib)
    got = P.optimize_windows_dev(torch.from_numpy(pred).to(dev), torch.from_numpy(vos).to(dev), True, 1, 1, 2.0, 1, 10, lib)
    assert torch.is_tensor(got) and got.dtype == torch.float64 and got.device.type == torch.device(dev).type
    assert np.array_equal(got.cpu().numpy(), want)
    try:
        P.optimize_windows_dev(torch.from_numpy(pred).to(dev), torch.from_numpy(vos[:, :3]).to(dev).contiguous(), True, binding=lib)
        raise AssertionError("a chain's VOs for a fully connected graph must be refused")
    except ValueError as e:
        assert "d_vos" in str(e)
    nan = pred.copy()
    nan[2] = np.nan
    try:
        P.optimize_windows_dev(torch.from_numpy(nan).to(dev), torch.from_numpy(vos).to(dev), True, binding=lib)
        raise AssertionError("a window that is not positive definite must raise")
    except np.linalg.LinAlgError as e:
        assert "[2]" in str(e)


# ---- the pose table -------------------------------------------------------------------------------------------------------------------
H, W_IMG, FRAMES, CHUNK = 32, 40, 7, 3


class Frames(torch.utils.data.Dataset):
    """a frame dataset without `poses`: (frame, pose) items only"""

    def __init__(self, frames, poses):
        self.frames, self._poses, self.gt_idx = frames, poses, np.arange(len(frames))

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[int(i)], self._poses[int(i)]


def _frames(form, n=FRAMES, seed=31):
    g = torch.Generator().manual_seed(seed)
    if form == "u8":
        return torch.randint(0, 256, (n, H, W_IMG, 3), generator=g, dtype=torch.uint8)
    return torch.randn(n, 3, H, W_IMG, generator=g)


def _traj(n, seed=31):
    return SyntheticFrames(n, H=8, W=8, seed=seed).poses


def _pair(lib, dev, dtype_name, form, fused):
    onet, net = IG.pair(lib, dev, dtype_name)
    if form == "u8":
        net.set_input_u8(MEAN, STD)
    if fused:
        net.set_eval_fused(True)
    return onet, net


class _Count:
    """wraps the engine's forward: counts the passes and their batch sizes"""

    def __init__(self, net):
        self.eng, self.sizes = net.mapnet._engine, []
        self._orig = self.eng.forward

    def __enter__(self):
        def forward(images, training):
            self.sizes.append(int(images.shape[0]))
            return self._orig(images, training)
        self.eng.forward = forward
        return self

    def __exit__(self, *exc):
        del self.eng.forward


def check_pose_table(lib, dev, dtype_name, form="fp32", fused=False):
    """predict_frames on 7 frames in chunks of 3 (3, 3, 1 padded), fed by a host dataset and by a resident view: three passes each,
    the same table bit for bit; its rows are those of the forward passes it stands for (fp32 frames; uint8 frames on the GPU, where a
    pass costs nothing -- the emulator spends 20 s on one); per frame within the pose bar of the oracle"""
    checks._fresh()
    onet, net = _pair(lib, dev, dtype_name, form, fused)
    x = _frames(form)
    xd = x.to(dev)
    data = Frames(x, _traj(FRAMES))  # a host dataset without `poses`
    with _Count(net) as c:
        table = E.predict_frames(net, x if form == "u8" else data, batch_frames=CHUNK)  # a tensor of frames, or a host dataset
    assert c.sizes == [CHUNK] * 3, c.sizes
    assert tuple(table.shape) == (FRAMES, 6) and table.dtype == torch.float32 and table.device.type == torch.device(dev).type
    t = table.cpu()
    assert torch.isfinite(t).all()
    if form == "fp32" or torch.device(dev).type == "cuda":
        with torch.no_grad():
            assert torch.equal(t[0:3], net.mapnet(xd[0:3].contiguous()).cpu())
            assert torch.equal(t[3:6], net.mapnet(xd[3:6].contiguous()).cpu())
            padded = xd[6:7].expand(CHUNK, *xd.shape[1:]).contiguous()
            assert torch.equal(t[6], net.mapnet(padded).cpu()[0])
    assert len(net.mapnet._engine.plans) == 1  # one plan served every chunk
    # a resident view (base 2: behind another dataset's frames), through the PoseNet under the MapNet, from training mode
    (view,) = ResidentFrames.build([Frames(_frames(form, 2, seed=1), _traj(2)), data], dev)[1:]
    assert view.base == 2
    net.train()
    with _Count(net) as c:
        assert torch.equal(E.predict_frames(net.mapnet, view, batch_frames=CHUNK).cpu(), t)
    assert c.sizes == [CHUNK] * 3
    assert net.training and net.mapnet.training  # the training flag is restored
    net.eval()
    if form == "fp32":
        with torch.no_grad():
            ref = onet.mapnet(x)
        err = (t - ref).abs().max().item()
        checks._record_deviation({"check": "pose_table", "dtype": dtype_name, "fused": fused, "dev": str(dev), "pose_abs_max": err,
                                  "scale": ref.abs().max().item()})
        assert err <= 1e-3 * max(1.0, ref.abs().max().item()), err


def check_refusals(lib, dev):
    checks._fresh()
    _, net = _pair(lib, dev, "fp32", "u8", False)
    x = _frames("u8")
    for bad in (0, -3):
        try:
            E.predict_frames(net, x, batch_frames=bad)
            raise AssertionError("batch_frames=%d must be refused" % bad)
        except ValueError as e:
            assert "batch_frames" in str(e)
    net.set_color_jitter(0.4, 0.4, 0.4, 0.1, seed=3)
    net.train()
    try:
        E.predict_frames(net, x, batch_frames=CHUNK)
        raise AssertionError("an active ColorJitter must be refused")
    except MapNetHipError as e:
        assert "one pose per frame" in str(e) and "ColorJitter" in str(e)
    assert net.training and not net.mapnet._engine.plans  # refused before anything ran
    net.set_color_jitter()
    net.eval()
    data = Frames(x, _traj(FRAMES))
    for vo_func, fc in ((calc_vos_safe, True), (calc_vos_safe_fc, False), (lambda p: p[:, 1:] - p[:, :-1], False)):
        mf = MF(data, steps=3, skip=2, include_vos=True, real=True, vo_func=vo_func, gt_dataset=data)
        try:
            E.evaluate_sequence(net, mf, pose_graph=True, fc_vos=fc, batch_frames=CHUNK)
            raise AssertionError("a vo_func the kernel does not restate must be refused")
        except ValueError as e:
            assert "vo_func" in str(e)
    try:
        E.evaluate_sequence(net, MF(data, steps=3, skip=2), pose_graph=True, batch_frames=CHUNK)
        raise AssertionError("pose_graph without VO targets must be refused")
    except ValueError as e:
        assert "include_vos" in str(e)
    assert not net.mapnet._engine.plans


# ---- against the window loop -----------------------------------------------------------------------------------------------------------
POSE_M, POSE_S = np.array([0.5, -1.0, 2.0]), np.array([2.0, 3.0, 0.5])  # checks.check_eval_flow's
LOOP_BATCH = 4  # 7 frames: a chunk of 4 and one of 3 padded; the loop forwards batches of `steps`


_SHARED = {}


def _shared(lib, dev, dtype_name, fused):
    """(oracle, model, frames x [7,3,32,40], frame dataset) of the loop checks: one model per (backend, dtype), so that on the
    emulator -- 20 s per forward pass, whatever its size -- a pass over the same frames is computed once (_Memo)"""
    import geomapnet_amd as G
    key = (id(lib), str(dev), dtype_name, fused)
    if key not in _SHARED:
        onet, net = _pair(lib, dev, dtype_name, "fp32", fused)
        x = _frames("fp32", seed=33)
        _SHARED[key] = (onet, net, x, Frames(x, _traj(FRAMES)), {})
    G.set_compute_dtype(dtype_name)  # (process-wide: another test may have changed it since)
    return _SHARED[key]


class _Memo:
    """emulator only: the engine's forward, remembered per input batch.  The window loop forwards the same seven windows in every
    check of this section; what is compared is which frames each path forwards and what it does with the poses, not whether two
    passes over the same batch agree"""

    def __init__(self, net, memo, dev):
        self.eng, self.memo, self.on = net.mapnet._engine, memo, torch.device(dev).type == "cpu"

    def __enter__(self):
        if self.on:
            orig = self.eng.forward

            def forward(images, training):
                key = (tuple(images.shape), bool(training), images.numpy().tobytes())
                if key not in self.memo:
                    self.memo[key] = orig(images, training)
                return self.memo[key].clone()
            self.eng.forward = forward
        return self

    def __exit__(self, *exc):
        if self.on:
            del self.eng.forward


def _loop(net, data_set, **kw):
    loader = torch.utils.data.DataLoader(data_set, batch_size=1, shuffle=False, num_workers=0)
    return E.evaluate(net, loader, POSE_M, POSE_S, cuda=True, **kw)


def check_against_loop(lib, dev, dtype_name, fused=False):
    """MF(steps=3, skip=2) over 7 frames: evaluate_sequence returns what evaluate returns"""
    checks._fresh()
    onet, net, x, data, memo = _shared(lib, dev, dtype_name, fused)
    mf = MF(data, steps=3, skip=2)
    with _Memo(net, memo, dev):
        s_loop, p_loop, t_loop = _loop(net, mf)
        s_seq, p_seq, t_seq = E.evaluate_sequence(net, mf, POSE_M, POSE_S, batch_frames=LOOP_BATCH)
    assert p_seq.shape == p_loop.shape == (FRAMES, 7) and t_seq.shape == t_loop.shape
    assert np.array_equal(t_seq, t_loop)
    with torch.no_grad():
        scale = max(1.0, onet.mapnet(x).abs().max().item())
    bound = 2 * 1e-3 * scale * POSE_S  # each path within the pose bar of the oracle; per column, un-normalised
    diff = np.abs(p_seq[:, :3] - p_loop[:, :3]).max(axis=0)
    checks._record_deviation({"check": "sequence_vs_loop", "dtype": dtype_name, "fused": fused, "dev": str(dev),
                              "t_abs_max": diff.tolist(), "bound": bound.tolist()})
    print("sequence vs loop (%s%s): translation columns differ by %s, bound %s" % (dtype_name, " fused" if fused else "", diff, bound))
    assert (diff <= bound).all(), (diff, bound)
    # PoseNet on a plain frame dataset: windows of one frame
    with _Memo(net, memo, dev):
        s1, p1, t1 = E.evaluate_sequence(net.mapnet, data, POSE_M, POSE_S, batch_frames=LOOP_BATCH)
    assert p1.shape == (FRAMES, 7) and np.array_equal(t1, E.to_pose7(_traj(FRAMES).numpy(), POSE_M, POSE_S))
    assert np.abs(p1[:, :3] - p_seq[:, :3]).max() == 0.0  # the same table, the frame itself in the middle


def check_against_loop_pose_graph(lib, dev, dtype_name, steps, fc, fused=False):
    """with pose_graph, scattered by get_indices: (i) the optimised windows are those of optimize_windows on the device-assembled
    poses7 / vos7 copied to the host; (ii) median_t / mean_t agree with evaluate(pose_graph=True)"""
    checks._fresh()
    _, net, _, data, memo = _shared(lib, dev, dtype_name, fused)
    gt = Frames(data.frames, _traj(FRAMES, seed=34))
    mf = MF(data, steps=steps, skip=2, include_vos=True, real=True, vo_func=calc_vos_safe_fc if fc else calc_vos_safe, gt_dataset=gt)
    sig = dict(sax=1.0, saq=1.0, srx=20.0, srq=20.0)
    with _Memo(net, memo, dev):
        s_loop, p_loop, t_loop = _loop(net, mf, pose_graph=True, fc_vos=fc, indices_of=mf.get_indices, length=len(mf), **sig)
    seen = []
    orig = E.windows_from_tables

    def spy(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]

    E.windows_from_tables = spy
    try:
        with _Memo(net, memo, dev):
            s_seq, p_seq, t_seq = E.evaluate_sequence(net, mf, POSE_M, POSE_S, pose_graph=True, fc_vos=fc, batch_frames=LOOP_BATCH,
                                                      scatter=True, **sig)
    finally:
        E.windows_from_tables = orig
    assert p_seq.shape == p_loop.shape == (FRAMES, 7) and np.array_equal(t_seq, t_loop)
    assert np.array_equal(t_seq, E.to_pose7(_traj(FRAMES, seed=34).numpy(), POSE_M, POSE_S))  # the ground-truth set's poses
    # (i)
    (d_poses7, d_vos7, d_bad), = seen
    assert tuple(d_poses7.shape) == (FRAMES, steps, 7) and d_bad.item() == 0.0
    opt = P.optimize_windows(d_poses7.cpu().numpy(), d_vos7.cpu().numpy(), fc_vos=fc, device=dev, binding=lib, **sig)
    opt[:, :, :3] = opt[:, :, :3] * POSE_S + POSE_M
    want = np.zeros((FRAMES, 7))
    for i in range(FRAMES):
        want[mf.get_indices(i)[steps // 2]] = opt[i, steps // 2]
    assert np.array_equal(p_seq, want)
    # (ii)
    got = np.array([s_seq["median_t"], s_seq["mean_t"]])
    ref = np.array([s_loop["median_t"], s_loop["mean_t"]])
    checks._record_deviation({"check": "sequence_vs_loop_pgo", "dtype": dtype_name, "fused": fused, "steps": steps, "fc": bool(fc),
                              "dev": str(dev), "max_abs_diff": float(np.abs(got - ref).max()),
                              "max_rel_diff": float((np.abs(got - ref) / (np.abs(ref) + 1e-12)).max())})
    print("sequence vs loop, pose graph (steps %d, fc %s, %s): median_t / mean_t %s vs %s" % (steps, fc, dtype_name, got, ref))
    np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-3)
