"""CPU: the pieces the three hipGraph front ends share -- ops.StepContext.scoped / unscoped, the scoping helpers of ops
written through them, and StartFeeder / LRU of sug_amd.graph_replay."""
import pytest
import torch

from sug_amd import ops
from sug_amd.graph_replay import LRU, StartFeeder, refusal_text, tensor_outputs


def test_scoped_sets_restores_and_nests():
    C = ops.StepContext()
    with C.scoped(bn_groups=2, w16_cache={}) as inside:
        assert inside is C and C.bn_groups == 2 and C.w16_cache == {}
        with C.scoped(bn_groups=3, fused_heads=True):
            assert C.bn_groups == 3 and C.fused_heads is True and C.w16_cache == {}
        assert C.bn_groups == 2 and C.fused_heads is False
    assert C.bn_groups == 1 and C.w16_cache is None


def test_scoped_restores_when_the_body_raises():
    C = ops.StepContext()
    C.start_provider = keep = lambda B, N: None
    with pytest.raises(KeyError):
        with C.scoped(start_provider=None, bn_groups=4):
            assert C.start_provider is None
            raise KeyError('body')
    assert C.start_provider is keep and C.bn_groups == 1


def test_scoped_rejects_an_unknown_field_and_sets_nothing():
    C = ops.StepContext()
    with pytest.raises(AttributeError):
        with C.scoped(bn_groups=2, no_such_field=1):
            pass
    assert C.bn_groups == 1


@pytest.mark.parametrize('field,value', [('bn_groups', 2), ('start_queue', []), ('geometry_plan', []),
                                         ('start_provider', lambda B, N: None), ('profile', {}), ('bn_record', [])])
def test_unscoped_is_false_while_a_blocking_field_is_set(field, value):
    C = ops.StepContext()
    assert C.unscoped()
    with C.scoped(**{field: value}):
        assert not C.unscoped()
    assert C.unscoped()


def test_unscoped_ignores_the_fields_a_capture_may_run_under():
    C = ops.StepContext()
    with C.scoped(fused_heads=True, parallel_branches=True, w16_cache={}, pending_counts={}, profile_only={'x'}):
        assert C.unscoped()


def test_ops_scoping_helpers_behave_as_before():
    assert ops.CTX.unscoped()
    with ops.bn_groups(2.0):
        assert ops.CTX.bn_groups == 2 and isinstance(ops.CTX.bn_groups, int)
        with ops.bn_groups(1):
            assert ops.CTX.bn_groups == 1
        assert ops.CTX.bn_groups == 2
    assert ops.CTX.bn_groups == 1
    mine = [torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.long)]
    with ops.start_queue(mine):
        assert ops.CTX.start_queue == mine and ops.CTX.start_queue is not mine
        assert ops.draw_start(2, 16) is mine[0]
        assert len(ops.CTX.start_queue) == 1 and len(mine) == 2        # the caller's list is not consumed
    assert ops.CTX.start_queue is None
    with ops.start_queue(None):
        assert ops.CTX.start_queue is None
    with ops.record_bn_stats() as outer:
        assert outer == [] and ops.CTX.bn_record is outer
        with ops.record_bn_stats() as inner:
            assert ops.CTX.bn_record is inner and inner is not outer
        assert ops.CTX.bn_record is outer
    assert ops.CTX.bn_record is None
    with pytest.raises(ZeroDivisionError):
        with ops.bn_groups(2), ops.record_bn_stats():
            1 / 0
    assert ops.CTX.unscoped()


def test_feeder_recording_collects_the_plan_and_restores_the_provider():
    fd = StartFeeder('cpu')
    with fd.recording():
        a, b = ops.draw_start(2, 16), ops.draw_start(3, 8)
    assert fd.plan == [(2, 16), (3, 8)] and ops.CTX.start_provider is None
    assert a.shape == (2,) and b.shape == (3,) and a.dtype == torch.long and int(a.max()) < 16 and int(b.max()) < 8
    with pytest.raises(KeyError):
        with fd.recording():
            raise KeyError('body')
    assert ops.CTX.start_provider is None


def _planned_feeder():
    fd = StartFeeder('cpu')
    fd.plan = [(2, 16), (3, 8)]
    fd.dev = torch.arange(5, dtype=torch.int32)         # (build() would pin host memory: a hand-made buffer instead)
    return fd


def test_feeder_providing_hands_out_consecutive_slices():
    fd = _planned_feeder()
    fd.cursor = 7                                       # left over from an earlier capture
    with fd.providing():
        a, b = ops.draw_start(2, 16), ops.draw_start(3, 8)
    assert a.tolist() == [0, 1] and b.tolist() == [2, 3, 4] and a.data_ptr() == fd.dev.data_ptr()
    assert fd.cursor == 2 and ops.CTX.start_provider is None


def test_feeder_providing_raises_on_an_under_draw():
    fd = _planned_feeder()
    with pytest.raises(RuntimeError, match='the captured forward drew 1 FPS starts, the eager one 2'):
        with fd.providing():
            ops.draw_start(2, 16)
    assert ops.CTX.start_provider is None


def test_feeder_providing_lets_the_bodys_exception_through():
    fd = _planned_feeder()
    with pytest.raises(KeyError, match='body'):         # not replaced by the draw-count error (no draw was taken)
        with fd.providing():
            raise KeyError('body')
    assert ops.CTX.start_provider is None
    with pytest.raises(AssertionError, match='forward structure changed'):
        with fd.providing():
            ops.draw_start(2, 17)
    assert ops.CTX.start_provider is None


def test_lru_bounds_evicts_the_least_recently_used_and_follows_its_limit():
    gone = []
    d = LRU(8, gone.append)
    for k in range(8):
        assert d.put(('k', k), k) == k
    assert d.get(('k', 0)) == 0                         # key 0 used again: key 1 is now the least recently used
    assert d.get(('k', 99)) is None and d.get(('k', 99), 5) == 5 and len(d) == 8 and not gone
    d.put(('k', 8), 8)
    assert len(d) == 8 and ('k', 1) not in d and ('k', 0) in d and ('k', 8) in d and gone == [1]
    d.limit = 2                                         # lowered after construction: holds from the next insertion
    assert len(d) == 8
    d.put(('k', 9), 9)
    assert list(d) == [('k', 8), ('k', 9)] and gone == [1, 2, 3, 4, 5, 6, 7, 0]
    plain = LRU(1)                                      # no eviction callback
    plain.put('a', 1)
    plain.put('b', 2)
    assert list(plain.items()) == [('b', 2)]


def test_refusal_text_and_tensor_outputs():
    assert refusal_text(RuntimeError('first line\nsecond')) == 'RuntimeError: first line'
    assert refusal_text(ValueError()) == 'ValueError: '
    t = torch.zeros(1)
    assert tensor_outputs(t) == ([t], True)
    outs, single = tensor_outputs((t, t))
    assert outs == [t, t] and isinstance(outs, list) and not single
    assert tensor_outputs(None) == ([], False)
