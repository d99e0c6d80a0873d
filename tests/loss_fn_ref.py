"""TEST INFRASTRUCTURE: the three pose criteria with pluggable loss modules (common/criterion.py:33-184: `t_loss_fn` /
`q_loss_fn`, and QuaternionLoss :15-31), restated in plain torch and differentiated by autograd -- float64 when the module and
its inputs are.  The parameters and the relative-pose chain are the oracle's (oracle/criterion.py, oracle/pose_math.py); only the
fixed L1 mean of oracle/criterion.py is replaced by the two modules.  tests/test_loss_fns.py pins this file to the reference's
own classes wherever the reference tree is present."""
import torch
from torch import nn

from oracle import pose_math
from oracle.criterion import _PoseCriterion


class QuaternionLoss(nn.Module):
    """common/criterion.py:15-31 with pose_utils.vdot (:21-30) written out"""

    def forward(self, q1, q2):
        return torch.mean(1 - torch.pow(torch.sum(torch.mul(q1, q2), 1), 2))


def _term(s, fn, a, b):
    return torch.exp(-s) * fn(a, b) + s


def _rows(x):
    return x.reshape(-1, x.shape[-1])


class _FnCriterion(_PoseCriterion):
    def __init__(self, t_loss_fn=None, q_loss_fn=None, **kw):
        super().__init__(**kw)
        self.t_loss_fn = nn.L1Loss() if t_loss_fn is None else t_loss_fn
        self.q_loss_fn = nn.L1Loss() if q_loss_fn is None else q_loss_fn

    def _abs(self, pred, targ):  # :48-51, :85-91, :159-163
        p, g = _rows(pred), _rows(targ)
        return _term(self.sax, self.t_loss_fn, p[:, :3], g[:, :3]) + _term(self.saq, self.q_loss_fn, p[:, 3:], g[:, 3:])

    def _vo(self, pv, gv):  # :99-105, :174-180
        pv, gv = _rows(pv), _rows(gv)
        return _term(self.srx, self.t_loss_fn, pv[:, :3], gv[:, :3]) + _term(self.srq, self.q_loss_fn, pv[:, 3:], gv[:, 3:])


class PoseNetCriterion(_FnCriterion):
    def __init__(self, t_loss_fn=None, q_loss_fn=None, sax=0.0, saq=0.0, learn_beta=False):
        super().__init__(t_loss_fn, q_loss_fn, sax=sax, saq=saq, learn_beta=learn_beta)

    def forward(self, pred, targ):
        return self._abs(pred, targ)


class MapNetCriterion(_FnCriterion):
    def __init__(self, t_loss_fn=None, q_loss_fn=None, sax=0.0, saq=0.0, srx=0.0, srq=0.0, learn_beta=False, learn_gamma=False):
        super().__init__(t_loss_fn, q_loss_fn, sax=sax, saq=saq, srx=srx, srq=srq, learn_beta=learn_beta, learn_gamma=learn_gamma)

    def forward(self, pred, targ):
        return self._abs(pred, targ) + self._vo(pose_math.calc_vos_simple(pred), pose_math.calc_vos_simple(targ))


class MapNetOnlineCriterion(_FnCriterion):
    def __init__(self, t_loss_fn=None, q_loss_fn=None, sax=0.0, saq=0.0, srx=0.0, srq=0.0, learn_beta=False, learn_gamma=False,
                 gps_mode=False):
        super().__init__(t_loss_fn, q_loss_fn, sax=sax, saq=saq, srx=srx, srq=srq, learn_beta=learn_beta, learn_gamma=learn_gamma)
        self.gps_mode = gps_mode

    def forward(self, pred, targ):
        T = pred.shape[1] // 2  # Python-2 integer division at :150
        loss = self._abs(pred[:, :T].contiguous(), targ[:, :T].contiguous())
        pv, gv = pred[:, T:].contiguous(), targ[:, T:].contiguous()
        if self.gps_mode:  # :173-176
            pv, gv = _rows(pv), _rows(gv)
            return loss + _term(self.srx, self.t_loss_fn, pv[:, :2], gv[:, :2])
        return loss + self._vo(pose_math.calc_vos(pv), gv)


MODES = ("posenet", "mapnet", "online", "gps")  # the library's modes 0-3


def make(mode, t_loss_fn=None, q_loss_fn=None, s4=(0.0, 0.0, 0.0, 0.0), learn=True):
    """the restated criterion of library mode 0-3"""
    kw = dict(sax=s4[0], saq=s4[1], learn_beta=learn)
    if mode == 0:
        return PoseNetCriterion(t_loss_fn, q_loss_fn, **kw)
    kw.update(srx=s4[2], srq=s4[3], learn_gamma=learn)
    if mode == 1:
        return MapNetCriterion(t_loss_fn, q_loss_fn, **kw)
    return MapNetOnlineCriterion(t_loss_fn, q_loss_fn, gps_mode=(mode == 3), **kw)


def differences(mode, pred, targ):
    """-> (translation, rotation) differences pred - targ of every element a per-element t_loss_fn / q_loss_fn sees in library
    mode 0-3 (absolute rows and VO rows together), each flattened: what beta / delta are chosen from"""
    pred, targ = pred.double(), targ.double()
    if mode == 0:
        d = [_rows(pred) - _rows(targ)]
    elif mode == 1:
        d = [_rows(pred) - _rows(targ), _rows(pose_math.calc_vos_simple(pred)) - _rows(pose_math.calc_vos_simple(targ))]
    else:
        T = pred.shape[1] // 2
        d = [_rows(pred[:, :T]) - _rows(targ[:, :T])]
        if mode == 2:
            d.append(_rows(pose_math.calc_vos(pred[:, T:])) - _rows(targ[:, T:]))
        else:
            d.append((_rows(pred[:, T:]) - _rows(targ[:, T:]))[:, :2])  # (two translation columns, no rotation)
    t = torch.cat([x[:, :3].reshape(-1) for x in d])
    q = torch.cat([x[:, 3:].reshape(-1) for x in d])
    return t, q
