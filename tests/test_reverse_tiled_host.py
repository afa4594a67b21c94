"""CPU checks of the tiled reverse-list build's host side: the header declares it, sug_reverse_lists_tiled_supported
answers on both sides of each limit, every refusal is an argument error before any launch (no device is needed to be
refused), and the reference of tests/reverse_tiled_cases.py equals a brute-force construction."""
import ctypes

import pytest
import torch

import reverse_tiled_cases as C


def test_header_declares_the_entry_points_and_the_limits():
    from sug_amd import _lib
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.DECLARATIONS['sug_reverse_lists_tiled_supported'] == (I, [I, I, I])
    assert _lib.DECLARATIONS['sug_reverse_lists_tiled'] == (I, [P, I, I, I, I, P, P, P])
    assert _lib.CONSTANTS['SUG_REV_TILED_MAX_DEST'] >= 32768
    assert _lib.CONSTANTS['SUG_REV_TILED_MAX_ENTRIES'] >= 2 ** 21
    assert _lib.CONSTANTS['SUG_REV_TILED_MAX_TILE'] % 1024 == 0 and _lib.CONSTANTS['SUG_REV_TILED_MAX_TILE'] >= 2048
    assert _lib.CONSTANTS['SUG_ABI_VERSION'] == 8 == _lib.lib().sug_abi_version()
    for name in ('sug_reverse_lists_tiled_supported', 'sug_reverse_lists_tiled'):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_supported_on_both_sides_of_each_limit():
    from sug_amd import _lib, ops
    ok = _lib.lib().sug_reverse_lists_tiled_supported
    maxn, maxe = _lib.CONSTANTS['SUG_REV_TILED_MAX_DEST'], _lib.CONSTANTS['SUG_REV_TILED_MAX_ENTRIES']
    for B in (1, 16, 64, 300):
        assert ok(B, 1, 1) == 1 and ok(B, 40960, 2048) == 1 and ok(B, 2 ** 21, 32768) == 1
        assert ok(B, maxe, maxn) == 1
        assert ok(B, maxe + 1, maxn) == 0 and ok(B, maxe, maxn + 1) == 0
        assert ok(B, 0, 8) == 0 and ok(B, 8, 0) == 0 and ok(B, -1, 8) == 0
    assert ok(0, 1024, 64) == 0 and ok(-3, 1024, 64) == 0
    assert ops.reverse_lists_tiled_supported(16, 40960, 2048) is True
    assert ops.reverse_lists_tiled_supported(0, 40960, 2048) is False


def test_every_refusal_is_an_argument_error_before_any_launch():
    from sug_amd import _lib
    L = _lib.lib()
    err = _lib.CONSTANTS['SUG_ERR_ARG']
    maxn, maxe = _lib.CONSTANTS['SUG_REV_TILED_MAX_DEST'], _lib.CONSTANTS['SUG_REV_TILED_MAX_ENTRIES']
    maxt = _lib.CONSTANTS['SUG_REV_TILED_MAX_TILE']
    p = ctypes.c_void_p(16)                      # never dereferenced: the checks come before the first HIP call
    for args in ((None, 2, 3000, 100, 0, p, p), (p, 2, 3000, 100, 0, None, p), (p, 2, 3000, 100, 0, p, None)):
        assert L.sug_reverse_lists_tiled(*args, None) == err and b'null' in L.sug_last_error()
    for tile in (1000, 1, -1024, 1536, maxt + 1024, maxt + 1):
        assert L.sug_reverse_lists_tiled(p, 2, 3000, 100, tile, p, p, None) == err
        msg = L.sug_last_error()
        assert b'tile=%d' % tile in msg and b'SUG_REV_TILED_MAX_TILE=%d' % maxt in msg, msg
    assert L.sug_reverse_lists_tiled(p, 2, 3000, maxn + 1, 0, p, p, None) == err
    assert b'SUG_REV_TILED_MAX_DEST=%d' % maxn in L.sug_last_error()
    assert L.sug_reverse_lists_tiled(p, 2, maxe + 1, 100, 0, p, p, None) == err
    assert b'SUG_REV_TILED_MAX_ENTRIES=%d' % maxe in L.sug_last_error()
    for B, E, N in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert L.sug_reverse_lists_tiled(p, B, E, N, 0, p, p, None) == err and b'bad shape' in L.sug_last_error()


def test_the_generic_build_keeps_its_limit():
    """sug_reverse_lists_build is not the dispatcher: one entry past its LDS formula is still refused."""
    import reverse_lists_cases as L0
    from sug_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    assert L.sug_reverse_lists_build(p, 2, 40960, 2048, 1, p, p, None) == _lib.CONSTANTS['SUG_ERR_ARG']
    assert b'too many' in L.sug_last_error()
    assert L0.lds_bytes(2, 40960, 2048)[0] > L0.LDS_LIMIT and L.sug_reverse_lists_tiled_supported(2, 40960, 2048) == 1


@pytest.mark.parametrize('case', ['partial_tile_few_dest', 'invalid_cloud'])
def test_reference_equals_per_destination_nonzero(case):
    idx = C.make(case)
    N = C.ALL[case][2]
    off, ent = C.reference(idx, N)
    assert off is not C.case_reference(case)[0] and torch.equal(off, C.case_reference(case)[0])
    for b in range(idx.shape[0]):
        at = 0
        for m in range(N):
            want = torch.nonzero(idx[b] == m).reshape(-1)
            assert int(off[b, m]) == at
            assert torch.equal(ent[b, at:at + want.numel()], want)
            at += want.numel()
        assert int(off[b, N]) == at == int(((idx[b] >= 0) & (idx[b] < N)).sum())
    if case == 'invalid_cloud':
        assert int(off[1].abs().sum()) == 0 and int(off[0, N]) == idx.shape[1]


def test_cases_are_what_their_names_say():
    """The patterns that aim at one part of the kernel do hit it (tile = 1024 entries)."""
    idx, N = C.make('gap'), C.ALL['gap'][2]
    d = N // 2
    per_tile = (idx == d).reshape(2, 3, 1024).sum(2)
    assert bool((per_tile[:, 0] > 0).all()) and bool((per_tile[:, 1] == 0).all()) and bool((per_tile[:, 2] > 0).all())
    idx, N = C.make('blocks'), C.ALL['blocks'][2]
    quarter = (idx // (N // 4)).reshape(2, 4, 1024)
    assert all(bool((quarter[:, t] == t).all()) for t in range(4))
    idx, N = C.make('one'), C.ALL['one'][2]
    assert idx.unique().tolist() == [N // 3] and idx.shape[1] > 4 * 1024
    idx, N = C.make('unlisted'), C.ALL['unlisted'][2]
    assert bool((idx % 2 == 0).all()) and int(idx.max()) < 2 * (N // 3)
    idx, N = C.make('invalid'), C.ALL['invalid'][2]
    bad = (idx < 0) | (idx >= N)
    assert 0.05 < float(bad.float().mean()) < 0.15 and {int(v) for v in idx[bad].unique()} == {-1, N, N + 5}
    idx = C.make('lists_of_768')
    assert torch.bincount(idx[0].long(), minlength=64).tolist() == [768] * 64
    assert C.ALL['n2048_k33-uniform'][1] > 65536 and C.ALL['n_at_the_limit'][2] == 32768
    for name, (B, E, N, tile, _, _) in C.CASES.items():
        assert tile in (1024, 2048), name
    for name in C.TILE_SWEEP:
        assert C.ALL[name][1] > 2048                                  # several tiles at both explicit sizes
