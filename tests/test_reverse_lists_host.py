"""CPU checks of tests/reverse_lists_cases.py: the argsort reference equals a brute-force construction, the restated
LDS formula gives the library's answers, and every case lies on the side of the 160 KB limit it is meant for."""
import ctypes

import pytest
import torch

import reverse_lists_cases as C


@pytest.mark.parametrize('case', C.SMALL)
def test_reference_equals_per_destination_nonzero(case):
    idx = C.make(case)
    N = C.SHAPES[C.CASES[case][0]][2]
    off, ent = C.reference(case)
    for b in range(idx.shape[0]):
        at = 0
        for m in range(N):
            want = torch.nonzero(idx[b] == m).reshape(-1)
            assert int(off[b, m]) == at
            assert torch.equal(ent[b, at:at + want.numel()], want)
            at += want.numel()
        assert int(off[b, N]) == at == int(((idx[b] >= 0) & (idx[b] < N)).sum())


def test_small_cases_cover_the_invalid_entries_and_the_patterns():
    assert {C.CASES[c][1] for c in C.SMALL} >= {'uniform', 'hubs', 'one', 'unlisted'}
    assert any(C.CASES[c][2] > 0 for c in C.SMALL)
    for c in C.CASES:
        if C.CASES[c][2] > 0:
            idx, N = C.make(c), C.SHAPES[C.CASES[c][0]][2]
            share = float(((idx < 0) | (idx >= N)).float().mean())
            assert 0.05 < share < 0.15 and {int(v) for v in idx[(idx < 0) | (idx >= N)].unique()} == {-1, N, N + 5}


def test_formula_restated_here_is_the_library_s():
    from sug_amd import _lib
    fits = _lib.lib().sug_scatter_rows_ordered_supported          # (B, N, E): sug_reverse_lists_lds_bytes <= 160 KB
    for B in (1, 2, 31, 32, 33, 64, 128, 300):
        for N in (1, 63, 64, 127, 128, 255, 256, 512, 1000, 1024, 2048, 5000):
            E = C.max_entries(B, N)
            assert fits(B, N, E) == 1 and fits(B, N, E + 1) == 0, (B, N, E)
            assert fits(B, N, 1) == 1


def test_every_case_is_on_its_side_of_the_limit():
    for name, (B, E, N, k) in C.SHAPES.items():
        assert C.lds_bytes(B, E, N)[0] <= C.LDS_LIMIT, name
        assert k is None or E == N * k
    for name in ('max_n512', 'max_n2048'):
        B, E, N, _ = C.SHAPES[name]
        assert E > 40000 and C.lds_bytes(B, E, N)[0] <= C.LDS_LIMIT < C.lds_bytes(B, E + 1, N)[0]
    assert C.lds_bytes(*C.SHAPES['bench'][:3]) == (4 * (2 * 256 + 32 + 20480), 4)


def test_one_entry_too_many_is_an_argument_error_before_any_launch():
    """No device is needed to be refused: the shape check comes before the first HIP call."""
    from sug_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int32 * 16)()
    for name in ('max_n512', 'max_n2048'):
        B, E, N, _ = C.SHAPES[name]
        rc = L.sug_reverse_lists_build(buf, B, E + 1, N, 1, buf, buf, None)
        assert rc == _lib.CONSTANTS['SUG_ERR_ARG'] and b'too many' in L.sug_last_error()
