"""CPU checks of tests/edgeconv_large_cases.py: the shape lies beyond the LDS-resident reverse-list build, the lists hold
what the docstring says, the probes zero few pairs, and the fp32 torch form keeps the margins for the chosen seed: where a
probe is not zero, it routes as the fp64 form does and stands on the same side of every activation kink."""
import torch

import dgcnn_seg_cases as D
import edgeconv_large_cases as E
import reverse_lists_cases as L0


def test_shape_is_beyond_the_lds_build_and_within_the_tiled_one():
    from sug_amd import ops
    assert E.N * E.K == 40960 and L0.lds_bytes(E.B, E.N * E.K, E.N)[0] > L0.LDS_LIMIT
    assert ops.reverse_lists_tiled_supported(E.B, E.N * E.K, E.N)
    assert L0.lds_bytes(64, 1024 * 20, 1024)[0] <= L0.LDS_LIMIT


def test_lists_have_two_hubs_and_unlisted_points():
    idx = E.inputs()['idx']
    assert tuple(idx.shape) == (E.B, E.N, E.K) and int(idx.min()) >= 0
    for b in range(E.B):
        counts = torch.bincount(idx[b].reshape(-1), minlength=E.N)
        assert int(counts[D.HUB]) >= 2 * E.N and int(counts[E.HUB2]) >= E.N // 2 - E.N // (E.K - 1) - 8
        assert int(counts[E.N - 1]) == 0 and int(counts[E.N - 2]) == 0
        assert int((counts == 0).sum()) >= 2


def test_probes_zero_few_pairs():
    lp, bp, (zl, zb) = E.probes()
    assert zl <= D.MAX_ZEROED and zb <= D.MAX_ZEROED, (zl, zb)
    assert float((lp != 0).double().mean()) > 0.98 and float((bp != 0).double().mean()) > 0.98


def test_fp32_torch_holds_the_margins_for_this_seed():
    lp, bp, _ = E.probes()
    r64, r32 = E.layer_reference('float64'), E.layer_reference('float32')
    live = lp != 0
    assert torch.equal(r64['nstar'][live], r32['nstar'][live])
    assert torch.equal(r64['pre'][live] > 0, r32['pre'][live] > 0)
    r64, r32 = E.block_reference('float64'), E.block_reference('float32')
    live = bp != 0
    assert torch.equal(r64['nstar'][live], r32['nstar'][live])
    assert torch.equal(r64['pre'][live] > 0, r32['pre'][live] > 0)
    # the first activation on the winning edges of the live pairs: channel c1 of edge (i, j*(c, i)) for every c1
    n = r64['nstar']                                                                   # [B,Co,N]
    for b in range(E.B):
        edges = torch.unique((torch.arange(E.N).view(1, E.N) * E.K + n[b])[live[b]])   # winning edges i * k + j
        s64 = r64['t1'][b].reshape(D.C1, -1)[:, edges] > 0
        s32 = r32['t1'][b].reshape(D.C1, -1)[:, edges] > 0
        assert torch.equal(s64, s32)
