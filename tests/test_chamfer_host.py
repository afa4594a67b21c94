"""CPU: the restatements the GPU tests of the ChamferDistance op rest on, the op's C ABI entries, and its refusals."""
import ctypes

import pytest
import torch

import chamfer_cases as C
from oracle import ref_cpu as O


def _double_loop(a, b):
    """dist / lowest index by a plain Python loop over fp32 scalars (numpy-free: torch 0-d fp32 arithmetic)."""
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    d = [[[None] * M for _ in range(N)] for _ in range(B)]
    for n in range(B):
        for i in range(N):
            for j in range(M):
                dx, dy, dz = (a[n, i, c] - b[n, j, c] for c in range(3))
                d[n][i][j] = ((dx * dx + dy * dy) + dz * dz).item()

    def side(rows):                                  # rows[q][c]: first strictly smaller wins -> the lowest index
        best, arg = [], []
        for row in rows:
            k = 0
            for c in range(1, len(row)):
                if row[c] < row[k]:
                    k = c
            best.append(row[k])
            arg.append(k)
        return best, arg

    out = [[], [], [], []]
    for n in range(B):
        d1, i1 = side(d[n])
        d2, i2 = side([[d[n][i][j] for i in range(N)] for j in range(M)])
        for o, v in zip(out, (d1, d2, i1, i2)):
            o.append(v)
    return (torch.tensor(out[0], dtype=torch.float32), torch.tensor(out[1], dtype=torch.float32),
            torch.tensor(out[2]), torch.tensor(out[3]))


@pytest.mark.parametrize('kind,B,N,M', [('random', 2, 5, 7), ('grid', 2, 6, 9), ('grid', 1, 1, 4), ('grid', 2, 11, 2)])
def test_fp32_restatement_against_a_double_loop(kind, B, N, M):
    a, b, got = C.case(kind, B, N, M)
    want = _double_loop(a, b)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    if kind == 'grid':
        t1, t2 = C.tie_counts(a, b)
        assert (t1 > 0 or M < 2) and (t2 > 0 or N < 2)


def test_grid_cases_tie_at_every_candidate_residue():
    """The tie cases of the GPU test do contain ties, and the tied candidates sit at different residues mod 8 (the split
    of a point's candidates over four lanes and two chains)."""
    for B, N, M in C.SHAPES:
        a, b, (_, _, idx1, idx2) = C.case('grid', B, N, M)
        t1, t2 = C.tie_counts(a, b)
        assert (t1 == B * N or M < 2) and (t2 == B * M or N < 2), (B, N, M, t1, t2)
    a, b, (_, _, idx1, _) = C.case('grid', 3, 257, 64)
    d = C.pair_sq_dist_fp32(a, b)
    tied = d == d.min(dim=2, keepdim=True).values                          # [B,N,M]
    res = torch.arange(64) % 8
    pairs = {(int(res[i]), int(r)) for row, i in zip(tied.reshape(-1, 64), idx1.reshape(-1)) for r in res[row] if int(r) != int(res[i])}
    assert {p[0] for p in pairs} == set(range(8)) and {p[1] for p in pairs} == set(range(8))


def test_fp32_restatement_against_the_oracle_chamfer():
    # both are fp32 sums of the same non-negative terms (each within a few roundings), in different orders
    for B, N, M in ((3, 257, 64), (3, 65, 9), (2, 1, 7)):
        a, b, (d1, d2, _, _) = C.case('random', B, N, M)
        want = O.chamfer_weights(a, b, 'none').reshape(-1)
        assert torch.allclose(d1.mean(1) + d2.mean(1), want, rtol=(max(N, M) + 8) * C.U, atol=0)


def test_fp64_restatement_is_the_gradient_of_its_own_loss():
    """Restatement (b) against autograd through a gather by the same indices (fp64)."""
    a, b, (_, _, idx1, idx2) = C.case('random', 2, 9, 5)
    g = torch.Generator().manual_seed(3)
    g1, g2 = torch.randn(2, 9, generator=g).double(), torch.randn(2, 5, generator=g).double()
    r = C.grads_fp64(a, b, idx1, idx2, g1, g2)
    A, Bt = a.double().requires_grad_(True), b.double().requires_grad_(True)
    d1 = ((A - torch.gather(Bt, 1, idx1[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    d2 = ((Bt - torch.gather(A, 1, idx2[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    ga, gb = torch.autograd.grad((d1 * g1).sum() + (d2 * g2).sum(), [A, Bt])
    assert torch.allclose(r['ga'], ga, rtol=1e-12, atol=1e-14) and torch.allclose(r['gb'], gb, rtol=1e-12, atol=1e-14)
    assert torch.allclose(r['dist1'], d1.detach()) and torch.allclose(r['dist2'], d2.detach())
    assert r['Ka'].sum().item() == 3 * 2 * 5 and r['Kb'].sum().item() == 3 * 2 * 9
    assert bool((r['Sa'] >= r['ga'].abs() - 1e-12).all())


def test_new_symbols_are_bound_with_their_types():
    from sug_amd import _lib
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES['sug_chamfer_nn'] == [P, P, I, I, I, P, P, P, P, P]
    assert _lib.SIGNATURES['sug_chamfer_nn_bwd'] == [P, P, P, P, P, P, I, I, I, P, P, P]
    assert _lib.CONSTANTS['SUG_CHAMFER_MAX_POINTS'] == 5000 and _lib.CONSTANTS['SUG_ABI_VERSION'] == 8
    L = _lib.lib()
    assert hasattr(L, 'sug_chamfer_nn') and hasattr(L, 'sug_chamfer_nn_bwd')


def test_shape_limits_are_checked_on_the_host():
    """Refused before any launch: safe without a GPU."""
    from sug_amd import _lib
    L = _lib.lib()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for B, N, M in ((1, 5001, 8), (1, 8, 5001), (1, 0, 8), (65536, 8, 8), (0, 8, 8)):
        assert L.sug_chamfer_nn(p, p, B, N, M, p, p, p, p, None) == -1
        assert b'sug_chamfer_nn: bad shape' in L.sug_last_error() and b'5000' in L.sug_last_error()
        assert L.sug_chamfer_nn_bwd(p, p, p, p, p, p, B, N, M, p, p, None) == -1
        assert b'sug_chamfer_nn_bwd: bad shape' in L.sug_last_error()
    assert L.sug_chamfer_nn(p, None, 1, 8, 8, p, p, p, p, None) == -1 and b'null' in L.sug_last_error()
    assert L.sug_chamfer_nn_bwd(p, p, p, p, p, None, 1, 8, 8, p, p, None) == -1 and b'null' in L.sug_last_error()


def test_cpu_tensors_are_refused():
    from sug_amd import ops
    from sug_amd.chamfer_distance import ChamferDistance, chamfer_distance
    from sug_amd.model import mmd
    assert mmd.ChamferDistance is ChamferDistance
    a, b = torch.zeros(1, 8, 3), torch.zeros(1, 4, 3)
    for f in (ops.chamfer_nn, ChamferDistance(), chamfer_distance):
        with pytest.raises(RuntimeError, match='HIP device'):
            f(a, b)
    with pytest.raises(RuntimeError, match='HIP device'):
        mmd.cd_distance(a, b, ChamferDistance(), batch_loss=False)
