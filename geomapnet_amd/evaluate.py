"""Evaluation flow and error metric of the reference (host side, fp64 numpy, as the reference computes it).

Mirrors /root/reference/scripts/eval.py:153-205 (inference loop, "take the middle prediction",
un-normalisation, error statistics) and the numpy helpers it uses from
/root/reference/common/pose_utils.py: `qexp` (:319-327), `quaternion_angular_error` (:361-371);
`t_criterion` is the L2 norm of eval.py:80.  The network forward inside the loop is the HIP path
(`step_feedfwd(train=False)`); pose-graph optimisation (eval.py:177-182, `--pose_graph`) runs on the HIP path
too, batched over all windows of the loop in one launch (geomapnet_amd/pgo.py).  `evaluate_sequence` is the same evaluation with
every frame forwarded once and the windows assembled on the device (csrc/seq_eval.h).
"""
import numpy as np

from .train import step_feedfwd


def qexp(q):
    """exponential map (3,) -> (4,): [cos n, sinc(n/pi) q]   (pose_utils.py:319-327)"""
    q = np.asarray(q)
    n = np.linalg.norm(q)
    return np.hstack((np.cos(n), np.sinc(n / np.pi) * q))


def quaternion_angular_error(q1, q2):
    """angular error between two quaternions in degrees   (pose_utils.py:361-371)"""
    d = abs(np.dot(q1, q2))
    d = min(1.0, max(-1.0, d))
    return 2 * np.arccos(d) * 180 / np.pi


def log_quaternion_angular_error(q1, q2):
    """pose_utils.py:358-359"""
    return quaternion_angular_error(qexp(q1), qexp(q2))


def t_criterion(t_pred, t_gt):
    """eval.py:80"""
    return np.linalg.norm(np.asarray(t_pred) - np.asarray(t_gt))


q_criterion = quaternion_angular_error


def to_pose7(logq_poses, pose_m, pose_s):
    """[M,6] (translation, log-quaternion) -> [M,7] (un-normalised translation, unit quaternion);
    eval.py:166-175 and :184-186"""
    p = np.asarray(logq_poses, dtype=np.float64).reshape(-1, 6)
    q = [qexp(r[3:]) for r in p]
    out = np.hstack((p[:, :3], np.asarray(q).reshape(-1, 4)))
    out[:, :3] = (out[:, :3] * np.asarray(pose_s, dtype=np.float64)) + np.asarray(pose_m, dtype=np.float64)
    return out


def pose_errors(pred_poses, targ_poses):
    """per-frame translation error (same unit as the poses) and rotation error (degrees) of [L,7] arrays
    (eval.py:192-196)"""
    t_loss = np.asarray([t_criterion(p, t) for p, t in zip(pred_poses[:, :3], targ_poses[:, :3])])
    q_loss = np.asarray([q_criterion(p, t) for p, t in zip(pred_poses[:, 3:], targ_poses[:, 3:])])
    return t_loss, q_loss


def summarize(t_loss, q_loss):
    """the numbers eval.py:202-205 prints"""
    return {"median_t": float(np.median(t_loss)), "mean_t": float(np.mean(t_loss)),
            "median_q": float(np.median(q_loss)), "mean_q": float(np.mean(q_loss))}


def evaluate(model, batches, pose_m=(0.0, 0.0, 0.0), pose_s=(1.0, 1.0, 1.0), cuda=True, pose_graph=False, fc_vos=False,
             sax=1, saq=1, srx=1, srq=1, indices_of=None, length=None):
    """Inference loop of eval.py:153-190.

    With `pose_graph` (eval.py:177-182) every target carries the window's VOs after its T absolute poses
    (`MF(include_vos=True)`: target [1,T+P,6]); predictions and VOs of all windows are collected and optimised by
    one `optimize_windows` launch, then un-normalised (eval.py:184-186 runs after the optimisation).

    `batches`: iterable of (data, target) as the reference's DataLoader yields them with batch_size 1:
    data [1,3,H,W] (PoseNet) or [1,T,3,H,W] (MapNet, `--model mapnet*`), target [1,6] / [1,T,6].  For
    every batch the MIDDLE prediction of the window is kept (eval.py:187-190: `output[len(output)/2]`).
    `indices_of(batch_idx)` (the MF dataset's `get_indices`, eval.py:158-163) with `length` = len(dataset): the middle
    prediction of batch i is WRITTEN at row `indices_of(i)[middle]` of zero-initialised [length, 7] arrays as the
    reference does -- windows clamped at the ends of a sequence repeat a middle index and overwrite each other, rows no
    window centres on stay zero -- instead of being appended one row per batch.
    Returns (summary dict, pred_poses [L,7], targ_poses [L,7])."""
    pred, targ, win_out, win_vos = [], [], [], []
    was_training = model.training
    model.eval()
    try:
        for data, target in batches:
            _, output = step_feedfwd(data, model, cuda, train=False)
            s = output.size()
            out = output.detach().cpu().numpy().reshape((-1, s[-1]))
            tgt = np.asarray(target.detach().cpu().numpy() if hasattr(target, "detach") else target).reshape((-1, s[-1]))
            if pose_graph:
                win_out.append(to_pose7(out, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))  # qexp only
                win_vos.append(to_pose7(tgt[len(out):], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
                tgt = tgt[:len(out)]
            else:
                out = to_pose7(out, pose_m, pose_s)
                pred.append(out[len(out) // 2])
            tgt = to_pose7(tgt, pose_m, pose_s)
            targ.append(tgt[len(tgt) // 2])
    finally:
        model.train(was_training)
    if pose_graph and win_out:
        from .pgo import optimize_windows
        from .posenet import engine_of
        eng = engine_of(model)  # the optimisation runs on the model's device, through the model's kernel library
        opt = optimize_windows(np.stack(win_out), np.stack(win_vos), fc_vos=fc_vos, sax=sax, saq=saq, srx=srx, srq=srq,
                               device=eng.device, binding=eng.lib)
        opt[:, :, :3] = (opt[:, :, :3] * np.asarray(pose_s, dtype=np.float64)) + np.asarray(pose_m, dtype=np.float64)
        pred = [o[len(o) // 2] for o in opt]
    return _scatter_and_summarize(np.asarray(pred), np.asarray(targ), indices_of, length)


def _scatter_and_summarize(pred_poses, targ_poses, indices_of, length):
    """the tail `evaluate` and `evaluate_sequence` share: one kept row per window -> (optionally) the rows of the windows' middle
    frames (eval.py:158-163), then the error statistics"""
    if indices_of is not None:
        n = int(length) if length is not None else len(pred_poses)
        pp, tp = np.zeros((n, 7)), np.zeros((n, 7))
        for i in range(len(pred_poses)):
            idx = list(indices_of(i))
            pp[idx[len(idx) // 2]] = pred_poses[i]
            tp[idx[len(idx) // 2]] = targ_poses[i]
        pred_poses, targ_poses = pp, tp
    t_loss, q_loss = pose_errors(pred_poses, targ_poses)
    return summarize(t_loss, q_loss), pred_poses, targ_poses


# ---- sequence evaluation: every frame forwarded once, windows and VOs assembled on the device ----------------------------------------
# In model.eval() BatchNorm runs on its running statistics, dropout never fires and a frame's pose does not depend on its batch
# mates: the loop's prediction for slot k of window i is the pose of frame get_indices(i)[k], whichever window asks.  One pose per
# frame (`predict_frames`) therefore holds everything the loop computes `steps` times over, and the windows, their VOs, the pose-graph
# optimisation and the error statistics are functions of that table (`evaluate_sequence`).  The one thing that breaks the premise is
# a per-pass random transform -- the device ColorJitter -- which is refused.
def predict_frames(model, frames, batch_frames=192):
    """One pose per frame: fp32 [L,6] on the model's device, row i = the eval-mode pose of frame i.

    `frames`: a frame dataset of (frame, pose) items, a `resident.ResidentFrames` view, or a tensor of frames ([L,3,H,W] fp32, or
    uint8 [L,h,w,3] after set_input_u8).  Chunks of `batch_frames` frames go through ONE plan: the last, partial chunk is padded by
    repeating its last frame (index) and the padded rows are dropped.  A view is fed as IndexedFrames(store, base + arange), 4 bytes
    per frame; a host dataset through a DataLoader (with DeviceFeed where the model is on a GPU).  No host synchronisation between
    chunks.  set_input_u8 / set_input_resize / set_eval_fused apply as in `model(x)`; a MapNet runs through the PoseNet under it."""
    import torch
    from ._binding import MapNetHipError
    from .feed import DeviceFeed
    from .posenet import MapNet, engine_of
    from .resident import IndexedFrames, ResidentFrames
    batch_frames = int(batch_frames)
    if batch_frames < 1:
        raise ValueError("predict_frames: batch_frames must be at least 1, got %d" % batch_frames)
    eng = engine_of(model)
    if eng.jitter_active():
        raise MapNetHipError("predict_frames: ColorJitter is active.  It draws fresh factors in every forward pass, so one pose per "
                             "frame is a different function from the loop's, which jitters a frame anew in every window; call "
                             "set_color_jitter() with all ranges 0 first, or use evaluate()")
    net = model.mapnet if isinstance(model, MapNet) else model
    dev = eng.device
    L = len(frames)
    if L < 1:
        raise ValueError("predict_frames: no frames")
    table = torch.empty(L, 6, dtype=torch.float32, device=dev)

    def chunks():
        """-> (first row, rows, batch of exactly batch_frames frames)"""
        if isinstance(frames, ResidentFrames):
            n_pad = -(-L // batch_frames) * batch_frames
            index = (frames.base + torch.arange(n_pad).clamp_(max=L - 1)).to(device=frames.store.device, dtype=torch.int32)
            for s in range(0, L, batch_frames):
                yield s, min(batch_frames, L - s), IndexedFrames(frames.store, index[s:s + batch_frames])
            return
        if torch.is_tensor(frames):
            batches = (frames[s:s + batch_frames] for s in range(0, L, batch_frames))
        else:
            loader = torch.utils.data.DataLoader(frames, batch_size=batch_frames, shuffle=False, num_workers=0,
                                                 pin_memory=dev.type == "cuda")
            batches = (b[0] for b in (DeviceFeed(loader, dev) if dev.type == "cuda" else loader))
        s = 0
        for x in batches:
            n = x.shape[0]
            x = x.to(dev, non_blocking=True)
            if n < batch_frames:
                x = torch.cat((x, x[-1:].expand(batch_frames - n, *x.shape[1:])), dim=0)
            yield s, n, x
            s += n

    was_training = model.training
    model.eval()
    try:
        for s, n, x in chunks():
            table[s:s + n].copy_(net(x)[:n])
    finally:
        model.train(was_training)
    return table


def _poses_of(dataset):
    """[L,6] poses of a frame dataset: its `poses`, or its items' once"""
    from .resident import _PosesOnly
    return _PosesOnly(dataset).poses


def windows_from_tables(lib, pose_table, vo_table, win, fc_vos=False):
    """mn_seq_windows (csrc/seq_eval.h) on the current stream, without a synchronisation: pose_table fp32 [L,6] on the device,
    vo_table [L,6] (any device; or None), win integer [W,N] -> (poses7 [W,N,7], vos7 [W,P,7] or None, bad flag [1]), fp64 tensors
    on pose_table's device: the inputs of `pgo.optimize_windows_dev`.  The flag reads 1 if an index of `win` lay outside [0, L)."""
    import ctypes as C
    import torch
    from ._binding import ptr
    dev = pose_table.device
    pose_table = pose_table.to(torch.float32).contiguous()
    L = int(pose_table.shape[0])
    d_win = torch.as_tensor(np.ascontiguousarray(win, dtype=np.int32)).to(dev)
    W, N = d_win.shape
    d_vo = d_vos7 = None
    if vo_table is not None:
        d_vo = torch.as_tensor(vo_table).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(d_vo.shape) != (L, 6):
            raise ValueError("windows_from_tables: vo_table must be [%d,6], got %s" % (L, list(d_vo.shape)))
        d_vos7 = torch.empty(W, N * (N - 1) // 2 if fc_vos else N - 1, 7, dtype=torch.float64, device=dev)
    d_poses7 = torch.empty(W, N, 7, dtype=torch.float64, device=dev)
    d_bad = torch.zeros(1, dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    lib.check(lib.seq_windows(ptr(pose_table), ptr(d_vo), ptr(d_win), L, W, N, 1 if fc_vos else 0, ptr(d_poses7), ptr(d_vos7),
                              ptr(d_bad), stream))
    return d_poses7, d_vos7, d_bad


def evaluate_sequence(model, data_set, pose_m=(0.0, 0.0, 0.0), pose_s=(1.0, 1.0, 1.0), cuda=True, pose_graph=False, fc_vos=False,
                      sax=1, saq=1, srx=1, srq=1, batch_frames=192, scatter=False):
    """`evaluate` over the batch-size-1 loader of `data_set` -- an `MF`, or a plain frame dataset (PoseNet: windows of one frame)
    -- with every frame forwarded once: (summary, pred_poses [.,7], targ_poses [.,7]) as `evaluate` returns them.

    The window matrix is `get_indices(i)` for i in range(len(data_set)), called once per window in order (variable_skip draws from
    numpy's generator as the loop does).  Targets are tables too: the absolute poses (`gt_dset.poses[gt_idx]` for a `real` dataset
    with VOs) and, as the source of the VOs, `data_set.dset`'s own poses -- what MF.__getitem__ hands to vo_func; no frame is read
    for either.  Without `pose_graph`: one device-to-host copy of the pose table, then to_pose7 of every window's middle row.  With
    it: mn_seq_windows assembles [W,N,7] predictions and [W,P,7] VOs on the device, `optimize_windows_dev` optimises them, the
    result is copied to the host and un-normalised.  The data set's vo_func must be calc_vos_safe (calc_vos_safe_fc with fc_vos):
    that is the function the kernel restates.  `scatter`: write each window's row at its middle frame's index (eval.py:158-163;
    `evaluate(indices_of=data_set.get_indices, length=len(data_set))`).  `cuda` is accepted for `evaluate`'s signature; the model's
    device decides.  Assumes what `predict_frames` assumes: eval mode, no per-pass random transform."""
    import torch
    from ._binding import MapNetHipError
    from .data import calc_vos_safe, calc_vos_safe_fc
    from .pgo import optimize_windows_dev
    from .posenet import engine_of
    windowed = hasattr(data_set, "get_indices") and hasattr(data_set, "dset")
    frames = data_set.dset if windowed else data_set
    include_vos = bool(windowed and data_set.include_vos)
    if pose_graph:
        if not include_vos:
            raise ValueError("evaluate_sequence: pose_graph needs an MF(include_vos=True) data set (the VOs are its targets)")
        want = calc_vos_safe_fc if fc_vos else calc_vos_safe
        if data_set.vo_func is not want:
            raise ValueError("evaluate_sequence: pose_graph with fc_vos=%s computes %s on the device; the data set's vo_func is %s"
                             % (bool(fc_vos), want.__name__, getattr(data_set.vo_func, "__name__", data_set.vo_func)))
    if windowed:
        win = np.stack([np.asarray(data_set.get_indices(i), dtype=np.int64) for i in range(len(data_set))])
    else:
        win = np.arange(len(data_set), dtype=np.int64)[:, None]
    W, N = win.shape
    mid = win[:, N // 2]
    # targets: absolute poses (MF.__getitem__: from the ground-truth dataset only for a `real` data set that carries VOs)
    if include_vos and data_set.real:
        targ_table = _poses_of(data_set.gt_dset)[torch.as_tensor(np.asarray(data_set.dset.gt_idx))]
    else:
        targ_table = _poses_of(frames)
    targ_table = np.asarray(targ_table)
    targ = to_pose7(targ_table[mid], pose_m, pose_s)

    table = predict_frames(model, frames, batch_frames)
    if not pose_graph:
        pred = to_pose7(table.cpu().numpy()[mid], pose_m, pose_s)
    else:
        lib = engine_of(model).lib
        d_poses7, d_vos7, d_bad = windows_from_tables(lib, table, _poses_of(frames), win, fc_vos)
        opt = optimize_windows_dev(d_poses7, d_vos7, fc_vos, sax, saq, srx, srq, binding=lib).cpu().numpy()
        if d_bad.item() != 0.0:  # (get_indices clips: only a data set whose frames and windows disagree gets here)
            raise MapNetHipError("evaluate_sequence: a window index lies outside the %d frames" % table.shape[0])
        opt[:, :, :3] = (opt[:, :, :3] * np.asarray(pose_s, dtype=np.float64)) + np.asarray(pose_m, dtype=np.float64)
        pred = opt[:, N // 2]
    return _scatter_and_summarize(pred, targ, (lambda i: win[i]) if scatter else None, W if scatter else None)


# ---- attention maps: the host side of scripts/plot_activations.py:134-143 of the reference ------------------------------------------
def _jet(v):
    """matplotlib's 'jet' colour map on values in [0, 1] -> RGB in [0, 1]; without matplotlib, the piecewise-linear segments jet is
    defined by (red 0.35-0.66-0.89-1, green 0.125-0.375-0.64-0.91, blue 0-0.11-0.34-0.65), un-quantised"""
    try:
        import matplotlib
        cm = matplotlib.colormaps["jet"] if hasattr(matplotlib, "colormaps") else __import__("matplotlib.cm").cm.get_cmap("jet")
        return np.asarray(cm(v))[..., :3]
    except ImportError:
        r = np.interp(v, [0.0, 0.35, 0.66, 0.89, 1.0], [0.0, 0.0, 1.0, 1.0, 0.5])
        g = np.interp(v, [0.0, 0.125, 0.375, 0.64, 0.91, 1.0], [0.0, 0.0, 1.0, 1.0, 0.0, 0.0])
        b = np.interp(v, [0.0, 0.11, 0.34, 0.65, 1.0], [0.5, 1.0, 1.0, 0.0, 0.0])
        return np.stack([r, g, b], axis=-1)


def attention_overlay(frame, amap, mean, std):
    """One frame of the attention video (plot_activations.py:134-143): jet(amap) * 255 blended 0.5 / 0.5 with the un-normalised
    frame, clipped to [0, 255], uint8 [H,W,3] in BGR order (what cv2.VideoWriter takes).
    frame: the normalised fp32 image [3,H,W] the network saw, or the uint8 frame [H,W,3]; amap: [H,W] in [0, 1] (PoseNet.saliency);
    mean, std: the Normalize statistics (3 values each; unused for a uint8 frame).
    As in the reference, the colour map's RGB triple is added to the image AFTER the image was flipped to BGR (its line 134 keeps
    cm_jet's channel order, line 140 flips the image only): in the written BGR frame jet's red end lands in the blue channel."""
    amap = np.asarray(amap, dtype=np.float64)
    frame = np.asarray(frame)
    if frame.dtype == np.uint8:
        img = frame.astype(np.float64)
    else:
        img = frame.astype(np.float64).transpose(1, 2, 0)
        img = (img * np.asarray(std, dtype=np.float64) + np.asarray(mean, dtype=np.float64)) * 255.0
    if img.shape[:2] != amap.shape:
        raise ValueError("attention_overlay: frame %s and map %s differ in size" % (img.shape[:2], amap.shape))
    act = _jet(np.clip(amap, 0.0, 1.0)) * 255.0
    out = 0.5 * img[:, :, ::-1] + 0.5 * act
    return np.clip(out, 0, 255).astype(np.uint8)
