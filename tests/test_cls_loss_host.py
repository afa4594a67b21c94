"""CPU: the host side of the fused classification-loss tail -- which criteria graph_replay.fused_criterion recognises, the
coefficients with which SUGStep hands its composed classification loss to ops.cls_loss, and the host-side validation of
sug_cls_loss_fwd / sug_cls_loss_bwd."""
import ctypes
import random

import pytest
import torch
import torch.nn as nn

from sug_amd.graph_replay import CriterionState, fused_criterion
from sug_amd.model.model_utils import focal_loss


def test_fused_criterion_recognises_plain_cross_entropy_only():
    assert fused_criterion(nn.CrossEntropyLoss(), 10) == ('ce', None, 0.0, 'mean', -100)
    assert fused_criterion(nn.CrossEntropyLoss(ignore_index=3), 10) == ('ce', None, 0.0, 'mean', 3)
    for c in (nn.CrossEntropyLoss(weight=torch.ones(10)), nn.CrossEntropyLoss(label_smoothing=0.1),
              nn.CrossEntropyLoss(reduction='sum'), nn.NLLLoss(), lambda p, y: p.sum()):
        assert fused_criterion(c, 10) is None


def test_fused_criterion_recognises_focal_loss_by_value():
    w = [0.05 * (i + 1) for i in range(10)]
    rec = fused_criterion(focal_loss(alpha=w, gamma=0, num_classes=10), 10)          # CLS_LOSS: ClassWeighting
    assert rec.kind == 'focal' and rec.gamma == 0.0 and rec.reduction == 'mean'
    assert rec.alpha == tuple(torch.tensor(w, dtype=torch.float32).tolist())
    rec = fused_criterion(focal_loss(gamma=2, num_classes=10, size_average=False), 10)   # CLS_LOSS: FocalLoss
    assert rec == ('focal', tuple(torch.Tensor([1 / 10] * 10).tolist()), 2.0, 'sum', -100)
    host = focal_loss(gamma=1.5, num_classes=10)
    host.alpha = torch.linspace(0.1, 1.0, 12)                                        # a host tensor, longer than C
    assert fused_criterion(host, 10).alpha == tuple(host.alpha.tolist()) and fused_criterion(host, 12) is not None
    assert fused_criterion(host, 13) is None                                         # fewer than C entries
    assert fused_criterion(focal_loss(gamma=2), 10) is None                          # (num_classes = 3 by default)


def test_fused_criterion_refuses_what_the_kernel_does_not_compute():
    class Sub(focal_loss):
        pass
    assert fused_criterion(Sub(gamma=2, num_classes=10), 10) is None                 # a subclass may compute anything
    assert fused_criterion(focal_loss(gamma=0.5, num_classes=10), 10) is None        # unbounded derivative at p_y = 1
    assert fused_criterion(focal_loss(gamma=-1, num_classes=10), 10) is None
    two_d = focal_loss(gamma=2, num_classes=10)
    two_d.alpha = torch.ones(2, 10)
    assert fused_criterion(two_d, 10) is None


def test_criterion_state_follows_the_criterion():
    st = CriterionState()
    c = focal_loss(gamma=2, num_classes=10)
    r0 = st.record(c)
    assert r0 == fused_criterion(c, 10) and st.record(c) is r0                       # unchanged: the same record, no new read
    c.gamma = 0
    assert st.record(c).gamma == 0.0
    c.alpha = torch.linspace(0.1, 1.0, 10)                                           # replaced ...
    r1 = st.record(c)
    assert r1.alpha == tuple(c.alpha.tolist())
    c.alpha[3] = 7.0                                                                 # ... and written in place
    assert st.record(c).alpha[3] == 7.0 and st.record(c) != r1
    assert st.record(nn.CrossEntropyLoss()).kind == 'ce' and st.record(nn.MSELoss()) is None
    assert st.alpha_on(st.record(nn.CrossEntropyLoss()), torch.device('cpu')) is None
    dev = st.alpha_on(r1, torch.device('cpu'))
    assert dev.dtype == torch.float32 and tuple(dev.tolist()) == r1.alpha and st.alpha_on(r1, torch.device('cpu')) is dev


def test_coefficients_reproduce_the_composed_classification_loss():
    """The composed block of SUGStep.losses on random scalars, in double arithmetic (a few ulp for the reassociation)."""
    from sug_amd.train_step import cls_loss_coefficients
    rnd = random.Random(7)
    for _ in range(200):
        M = {'CLS_WEIGHT': rnd.uniform(0.1, 3), 'SRC_LOSS_WEIGHT': rnd.uniform(0.1, 3),
             'ADV_WEIGHT': rnd.choice([0.0, -1.0, rnd.uniform(0.1, 2)]), 'TARGET_LOSS': rnd.choice([0.0, 1.0, rnd.uniform(0.1, 2)])}
        cs1, cs2, ct1, ct2, D = (rnd.uniform(0, 5) for _ in range(5))
        loss_s = 0.5 * (cs1 + cs2)                                  # train_step.py: the composed block, term for term
        if M['ADV_WEIGHT'] > 0:
            loss_s = loss_s - M['ADV_WEIGHT'] * D
        if M['TARGET_LOSS'] > 0:
            loss = 0.5 * (loss_s + 0.5 * (ct1 + ct2))
        else:
            loss = M['SRC_LOSS_WEIGHT'] * loss_s
        ref = M['CLS_WEIGHT'] * loss
        a_s, a_t, a_d = cls_loss_coefficients(M)
        got = a_s * (cs1 + cs2) + a_t * (ct1 + ct2) - a_d * D
        assert abs(got - ref) <= 8 * 2.0 ** -52 * max(1.0, abs(ref)), (M, got, ref)
        assert (a_t != 0) == (M['TARGET_LOSS'] > 0) and (a_d != 0) == (M['ADV_WEIGHT'] > 0)
    assert cls_loss_coefficients({'CLS_WEIGHT': 2.0, 'SRC_LOSS_WEIGHT': 3.0, 'ADV_WEIGHT': 0.5, 'TARGET_LOSS': 1.0}) == (0.5, 0.5, 0.5)
    assert cls_loss_coefficients({'CLS_WEIGHT': 2.0, 'SRC_LOSS_WEIGHT': 3.0, 'ADV_WEIGHT': 0.5, 'TARGET_LOSS': 0.0}) == (3.0, 0.0, 3.0)


def test_cls_loss_entry_points_validate_on_the_host():
    """Argument validation happens before any launch: safe without a GPU."""
    from sug_amd import _lib
    L = _lib.lib()
    f = ctypes.c_void_p(16)

    def fwd(p=f, C=10, gamma=2.0, a_t=0.0, a_d=0.0, lt=None, yt=f, Ms=4, Mt=4, ld=None):
        return L.sug_cls_loss_fwd(p, f, yt, yt, C if ld is None else ld, f, lt, Ms, Mt, C, None, gamma, 0, -100, 1.0, a_t, a_d, 1.0, f, f,
                                  None, None)

    def bwd(p=f, C=10, gamma=2.0, a_t=0.0, a_d=0.0, lt=None, yt=f, Ms=4, Mt=4, ld=None):
        return L.sug_cls_loss_bwd(f, f, yt, yt, C if ld is None else ld, f, lt, Ms, Mt, C, None, gamma, 0, -100, 1.0, a_t, a_d, 1.0, f, f,
                                  p, f, f, f, None)
    for call, name in ((fwd, b'sug_cls_loss_fwd'), (bwd, b'sug_cls_loss_bwd')):
        assert call(p=None) == -1
        assert b'null' in L.sug_last_error() and name in L.sug_last_error()
        assert call(a_t=0.25) == -1 and b'null' in L.sug_last_error()           # the target loss needs the target rows' labels
        assert call(a_d=1.0, yt=None) == -1 and b'null' in L.sug_last_error()   # the discrepancy needs the target rows
        assert call(C=65) == -1
        assert b'C=65' in L.sug_last_error() and name in L.sug_last_error()
        assert call(gamma=0.5) == -1
        assert b'gamma=0.5' in L.sug_last_error() and name in L.sug_last_error()
        assert call(gamma=-2.0) == -1 and call(gamma=float('nan')) == -1 and call(gamma=float('inf')) == -1
        assert call(Ms=0) == -1 and call(Mt=1025) == -1 and call(C=1) == -1 and call(ld=8) == -1     # ld < C
        assert call(a_d=float('nan')) == -1 and b'NaN' in L.sug_last_error()


def test_cls_loss_supported_says_no_without_raising():
    from sug_amd import ops
    y = torch.zeros(4, 10)
    assert not ops.cls_loss_supported(y, y, y, y)           # not on a HIP device: "not supported", the step composes the ops
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.cls_loss(y, y, y, y, torch.zeros(4, dtype=torch.long))
