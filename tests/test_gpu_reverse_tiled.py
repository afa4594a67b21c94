"""The tiled reverse-list build against the stable argsort (tests/reverse_tiled_cases.py): exact equality of rev_off and
of the valid part of rev_ent, a sentinel behind the valid count that must survive, at every tile size a case names, at
the sizes the LDS-resident build refuses, on the LDS build's own cases, and replayed from a captured graph."""
import pytest
import torch

import reverse_lists_cases as L0
import reverse_tiled_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _build(idx, N, tile):
    from sug_amd import ops
    ent = torch.full(idx.shape, SENTINEL, dtype=torch.int32, device='cuda')
    off, ent = ops.reverse_lists_tiled(idx.cuda(), N, tile=tile, ent=ent)
    return off.cpu().long(), ent.cpu().long()


def _check(off, ent, want_off, want_ent, N):
    E = ent.shape[1]
    assert torch.equal(off, want_off)
    valid = torch.arange(E).reshape(1, E) < want_off[:, N:N + 1]
    assert torch.equal(ent[valid], want_ent[valid])
    assert bool((ent[~valid] == SENTINEL).all()), 'rev_ent was written behind the valid entries'


@pytest.mark.parametrize('case', list(C.CASES))
def test_lists_equal_the_stable_argsort(case):
    B, E, N, tile = C.CASES[case][:4]
    off, ent = _build(C.make(case), N, tile)
    _check(off, ent, *C.case_reference(case), N)
    if case == 'invalid_cloud':
        assert int(off[1].abs().sum()) == 0 and bool((ent[1] == SENTINEL).all())


@pytest.mark.parametrize('case', list(C.REAL))
def test_sizes_beyond_the_lds_build_at_the_default_tile(case):
    B, E, N, tile = C.REAL[case][:4]
    assert tile == 0 and (E >= 65536 or L0.lds_bytes(B, E, N)[0] > L0.LDS_LIMIT)
    off, ent = _build(C.make(case), N, 0)
    _check(off, ent, *C.case_reference(case), N)


@pytest.mark.parametrize('case', list(L0.CASES))
def test_the_lds_build_s_cases_through_the_tiled_entry_point(case):
    """Equal to reverse_lists_cases.reference, which the LDS build is held to: the two builds give the same lists."""
    idx = L0.make(case)
    N = L0.SHAPES[L0.CASES[case][0]][2]
    off, ent = _build(idx, N, 1024)
    _check(off, ent, *L0.reference(case), N)


@pytest.mark.parametrize('case', C.TILE_SWEEP)
def test_every_tile_size_gives_the_same_arrays(case):
    N = C.CASES[case][2]
    got = [_build(C.make(case), N, tile) for tile in (1024, 2048, 0)]
    for off, ent in got:
        _check(off, ent, *C.case_reference(case), N)
        assert torch.equal(off, got[0][0]) and torch.equal(ent, got[0][1])


def test_two_builds_give_equal_bytes():
    N = C.REAL['n2048_k20-hubs'][2]
    a, b = _build(C.make('n2048_k20-hubs'), N, 0), _build(C.make('n2048_k20-hubs'), N, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals_launch_nothing():
    from sug_amd import ops, _lib
    idx = torch.zeros(2, 3000, dtype=torch.int32, device='cuda')
    ent = torch.full((2, 3000), SENTINEL, dtype=torch.int32, device='cuda')
    for tile in (1000, _lib.CONSTANTS['SUG_REV_TILED_MAX_TILE'] + 1024):
        with pytest.raises(RuntimeError, match='tile=%d' % tile):
            ops.reverse_lists_tiled(idx, 100, tile=tile, ent=ent)
    with pytest.raises(RuntimeError, match='SUG_REV_TILED_MAX_DEST'):
        ops.reverse_lists_tiled(idx, _lib.CONSTANTS['SUG_REV_TILED_MAX_DEST'] + 1, ent=ent)
    torch.cuda.synchronize()
    assert bool((ent == SENTINEL).all())


def test_replay_from_a_captured_graph_follows_idx():
    """One launch, no workspace, no host wait: captured on a side stream, replayed after idx was overwritten in place."""
    from sug_amd import ops
    B, E, N, tile, pattern, invalid = C.CASES['ragged']
    first, second = C.make('ragged'), C.draw(B, E, N, 'hubs', 0.1, 4242)
    assert not torch.equal(first, second)
    idx = first.cuda()
    ent = torch.full((B, E), SENTINEL, dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.reverse_lists_tiled(idx, N, tile=tile, ent=ent)           # warm: the LDS opt-in is taken outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard(), torch.cuda.graph(graph, stream=side):
        off, ent = ops.reverse_lists_tiled(idx, N, tile=tile, ent=ent)
    idx.copy_(second.cuda())
    ent.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    _check(off.cpu().long(), ent.cpu().long(), *C.reference(second, N), N)
