"""The reverse-list build against the stable argsort (tests/reverse_lists_cases.py): exact equality of rev_off and of
the valid part of rev_ent for every case, through ops.reverse_lists and, where E = N * k, through ops.knn_reverse."""
import pytest
import torch

import reverse_lists_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _build(case, sorted=True):
    from sug_amd import ops
    idx = C.make(case)
    N = C.SHAPES[C.CASES[case][0]][2]
    ent = torch.full(idx.shape, SENTINEL, dtype=torch.int32, device='cuda')
    off, ent = ops.reverse_lists(idx.cuda(), N, sorted=sorted, ent=ent)
    return idx, N, off.cpu().long(), ent.cpu().long()


def _valid_mask(off, N, E):
    return torch.arange(E).reshape(1, E) < off[:, N:N + 1]


@pytest.mark.parametrize('case', list(C.CASES))
def test_lists_equal_the_stable_argsort(case):
    idx, N, off, ent = _build(case)
    want_off, want_ent = C.reference(case)
    assert torch.equal(off, want_off)
    valid = _valid_mask(want_off, N, idx.shape[1])
    assert torch.equal(ent[valid], want_ent[valid])
    assert bool((ent[~valid] == SENTINEL).all()), 'rev_ent was written behind the valid entries'


@pytest.mark.parametrize('case', [c for c in C.CASES if C.SHAPES[C.CASES[c][0]][3] is not None])
def test_knn_reverse_gives_the_same_lists(case):
    from sug_amd import ops
    idx = C.make(case)
    B, E, N, k = C.SHAPES[C.CASES[case][0]]
    off, ent = ops.knn_reverse(idx.reshape(B, N, k).cuda())
    want_off, want_ent = C.reference(case)
    assert torch.equal(off.cpu().long(), want_off)
    valid = _valid_mask(want_off, N, E)
    assert torch.equal(ent.cpu().long()[valid], want_ent[valid])


@pytest.mark.parametrize('case', ['few_dest-invalid', 'ragged_ranges-hubs', 'interp-uniform', 'sparse-uniform', 'max_n512-one'])
def test_unsorted_lists_hold_the_same_entries(case):
    """sorted = 0: every destination's list, in whatever order, is the reference's list as a set."""
    idx, N, off, ent = _build(case, sorted=False)
    want_off, want_ent = C.reference(case)
    assert torch.equal(off, want_off)
    E = idx.shape[1]
    valid = _valid_mask(want_off, N, E)
    assert bool((ent[~valid] == SENTINEL).all())
    for b in range(idx.shape[0]):
        got, want = ent[b][valid[b]], want_ent[b][valid[b]]
        assert bool(((got >= 0) & (got < E)).all())
        dest = idx[b].long()
        assert torch.equal(dest[got], dest[want]), 'an entry lies in the list of another destination'
        assert torch.equal((dest[got] * E + got).sort()[0], dest[want] * E + want)


@pytest.mark.parametrize('case', ['max_n512-uniform', 'max_n2048-uniform'])
def test_one_entry_more_than_the_formula_accepts_is_refused(case):
    from sug_amd import ops
    B, E, N, _ = C.SHAPES[C.CASES[case][0]]
    idx = torch.zeros(B, E + 1, dtype=torch.int32, device='cuda')
    ent = torch.full((B, E + 1), SENTINEL, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='too many'):
        ops.reverse_lists(idx, N, ent=ent)
    torch.cuda.synchronize()
    assert bool((ent == SENTINEL).all()), 'a refused shape must launch nothing'


@pytest.mark.parametrize('case', ['ragged_ranges-hubs', 'interp-invalid', 'bench-uniform'])
def test_two_builds_give_equal_bytes(case):
    _, _, off1, ent1 = _build(case)
    _, _, off2, ent2 = _build(case)
    assert torch.equal(off1, off2) and torch.equal(ent1, ent2)
