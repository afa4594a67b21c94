"""Host side of the source-only training step (sug_amd.source_step.SourceStep, ops.ce, sug_ce_fwd / sug_ce_bwd): ABI
declarations, argument validation before any launch, the GPU-only messages and the learning-rate schedule.  No GPU."""
import warnings

import pytest
import torch


def test_ce_ctypes_signatures_match_header():
    """The binding is derived from the header; these lists are written by hand from the two prototypes."""
    from sug_amd._lib import SIGNATURES, _vp, _i32, _i64, _f32
    #                               logits ld  label M    C    ignore_index label_smoothing
    assert SIGNATURES['sug_ce_fwd'] == [_vp, _i64, _vp, _i32, _i32, _i64, _f32, _vp, _vp, _vp, _vp]     # loss lse totals stream
    assert SIGNATURES['sug_ce_bwd'] == [_vp, _i64, _vp, _i32, _i32, _i64, _f32, _vp, _vp, _vp, _vp]     # g lse dlogits stream


@pytest.mark.parametrize('M,C', [(1025, 10), (4, 65), (4, 1), (0, 10)])
def test_ce_fwd_range_is_checked_on_the_host(M, C):
    """Outside 1 <= M <= 1024, 2 <= C <= 64 the call returns -1 with sug_last_error() set before any launch (null
    pointers, no device needed)."""
    from sug_amd import _lib
    L = _lib.lib()
    assert L.sug_ce_fwd(None, max(C, 1), None, M, C, -100, 0.0, None, None, None, None) == -1
    msg = L.sug_last_error()
    assert b'sug_ce_fwd' in msg and b'unsupported shape' in msg
    assert L.sug_ce_bwd(None, max(C, 1), None, M, C, -100, 0.0, None, None, None, None) == -1
    assert b'sug_ce_bwd' in L.sug_last_error()


def test_ce_on_cpu_tensors_raises_gpu_only_message():
    from sug_amd import ops
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.ce(torch.zeros(4, 10), torch.zeros(4, dtype=torch.long))


@pytest.mark.parametrize('use_graph', [False, True])
def test_source_step_on_cpu_tensors_raises_gpu_only_message(use_graph):
    from sug_amd.model.model_pointnet import Pointnet_cls
    from sug_amd.source_step import SourceStep
    tr = SourceStep(Pointnet_cls(), use_graph=use_graph)
    with pytest.raises(RuntimeError, match='HIP device'):
        tr.step(torch.zeros(2, 3, 64, 1), torch.zeros(2, dtype=torch.long))


def test_set_epoch_is_cosine_annealing_stepped_with_explicit_epochs():
    """train_source.py:96, :106: CosineAnnealingLR(T_max=50).step(epoch=epoch)."""
    from sug_amd.model.model_pointnet import Pointnet_cls
    from sug_amd.source_step import SourceStep
    tr = SourceStep(Pointnet_cls(), lr=1e-3)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=50)
    for epoch in (0, 1, 7, 49, 50):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                 # the explicit-epoch form is deprecated in torch, not removed
            sched.step(epoch)
        want = opt.param_groups[0]['lr']
        got = tr.set_epoch(epoch, 50)
        assert got == pytest.approx(want, rel=1e-12, abs=1e-18), (epoch, got, want)
        assert all(g['lr'] == got for g in tr.optimizer.param_groups)


def test_kpfcls_is_declared_not_capturable():
    from sug_amd.model.KPConv_model import KPFCls
    assert KPFCls.graph_capturable is False
