"""CPU: argument checks of sug_eval_accumulate, the end-of-loop assembly of eval_worker from its accumulators, and the
key / runner bookkeeping of sug_amd.eval_graphs."""
import ctypes

import numpy as np
import pytest


def test_eval_accumulate_rejects_bad_arguments_on_the_host():
    from sug_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    args = lambda B, C, state: (p, None, C, p, B, C, None, 1, -100, 0.0, None, None, 1, state, 4, None)
    assert L.sug_eval_accumulate(*args(8, 10, None)) == -1
    assert b'null state' in L.sug_last_error()
    assert L.sug_eval_accumulate(*args(8, 65, p)) == -1
    assert b'C=65' in L.sug_last_error()
    assert L.sug_eval_accumulate(*args(4097, 10, p)) == -1
    assert b'B=4097' in L.sug_last_error()
    # the caller's loss scalar is required when the cross entropy is not fused
    a = list(args(8, 10, p))
    a[7] = 0
    assert L.sug_eval_accumulate(*a) == -1 and b'loss_in' in L.sug_last_error()


def _fold(batches, num_class, per_class):
    """What the kernel's thread 0 accumulates over the batches: (class_acc [64, 2], batch_acc)."""
    acc = np.zeros((64, 2))
    ratios = []
    for rows, correct in batches:             # per-class rows / correct rows of one batch
        if per_class:
            for c in range(num_class):
                if rows[c] > 0:
                    acc[c, 0] += float(correct[c]) / float(rows[c])
                    acc[c, 1] += 1.0
        ratios.append(float(sum(correct)) / float(sum(rows)))
    return acc, ratios


def _numpy_restatement(batches, num_class, per_class):
    acc = np.zeros((num_class, 3))
    ratios = []
    for rows, correct in batches:
        if per_class:
            for j in np.unique(np.repeat(np.arange(num_class), rows)):
                acc[j, 0] += correct[j] / float(rows[j])
                acc[j, 1] += 1
        ratios.append(sum(correct) / float(sum(rows)))
    with np.errstate(invalid='ignore', divide='ignore'):
        acc[:, 2] = acc[:, 0] / acc[:, 1]
    return acc, np.mean(acc[:, 2]), np.mean(ratios)


@pytest.mark.parametrize('source_flag,cls_eval', [(False, True), (False, False), (True, False)])
def test_assembly_matches_numpy_bit_for_bit(source_flag, cls_eval):
    from sug_amd.utils.eval_utils import assemble
    rng = np.random.default_rng(3)
    num_class = 10
    batches = []
    for b in range(23):
        rows = rng.integers(0, 5, num_class)
        rows[7] = 0                                   # class 7 never seen: NaN
        if rows.sum() == 0:
            rows[0] = 1
        correct = np.array([rng.integers(0, r + 1) for r in rows])
        batches.append((rows, correct))
    per_class = source_flag or cls_eval
    acc2, ratios = _fold(batches, num_class, per_class)
    class_acc, mean, inst = assemble(acc2, ratios, num_class)
    ref_acc, ref_mean, ref_inst = _numpy_restatement(batches, num_class, per_class)
    np.testing.assert_array_equal(class_acc, ref_acc)
    assert np.array_equal(mean, ref_mean, equal_nan=True)
    assert inst == ref_inst
    assert np.isnan(class_acc[7, 2])
    if not per_class:
        assert np.isnan(class_acc[:, 2]).all()
    else:
        assert not np.isnan(class_acc[:7, 2]).any()


def test_runner_keys_are_lru_bounded_and_signatures_cover_shapes_and_gemm_dtype(monkeypatch):
    import torch
    from sug_amd import eval_graphs
    from sug_amd.model import Ptran_transformer as PT
    from sug_amd.model.model_pointnet import Pointnet_cls
    net = Pointnet_cls().eval()
    r = eval_graphs.EvalRunner(net)
    for k in range(8):
        r.key_state(('k', k))
    r.key_state(('k', 0))                              # key 0 used again: key 1 is now the least recently used
    assert len(r.keys) == 8
    r.key_state(('k', 8))
    assert len(r.keys) == 8 and ('k', 1) not in r.keys and ('k', 0) in r.keys and ('k', 8) in r.keys
    assert r.stats['evicted'] == 1
    # signatures
    s0 = eval_graphs.signature(net)
    assert eval_graphs.signature(Pointnet_cls().eval()) == s0
    assert eval_graphs.signature(Pointnet_cls(num_class=12)) != s0
    monkeypatch.setattr(PT, 'GEMM_DTYPE', torch.float16)
    assert eval_graphs.signature(net) != s0
    # the private copy keeps no caches of the original
    assert '_call_graph_mgr' not in r.net.__dict__
    assert all(not getattr(m, 'cache_weight_split', False) for m in r.net.modules())


def test_runner_registry_keeps_two_signatures():
    from sug_amd import eval_graphs
    from sug_amd.model.model_pointnet import Pointnet_cls
    eval_graphs.drop_all()
    nets = [Pointnet_cls(num_class=c).eval() for c in (10, 11, 12)]
    rs = [eval_graphs.runner_for(n) for n in nets]
    assert eval_graphs.runner_for(nets[2]) is rs[2]
    assert len(eval_graphs._RUNNERS) == 2 and rs[0].sig not in eval_graphs._RUNNERS
    eval_graphs.drop_all()
