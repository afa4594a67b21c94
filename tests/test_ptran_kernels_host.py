"""CPU checks of tests/ptran_kernel_cases.py: the fp64 restatements that the GPU kernel tests are held against equal
the oracle's TransformerBlock, and the case generators deliver the regimes and neighbour lists they promise."""
import numpy as np
import pytest
import torch

import ptran_kernel_cases as C
from oracle import ref_cpu as O


def _state(dp, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {'fc1.weight': (512, dp), 'fc1.bias': (512,), 'fc2.weight': (dp, 512), 'fc2.bias': (dp,),
              'fc_delta.0.weight': (512, 3), 'fc_delta.0.bias': (512,), 'fc_delta.2.weight': (512, 512),
              'fc_delta.2.bias': (512,), 'fc_gamma.0.weight': (512, 512), 'fc_gamma.0.bias': (512,),
              'fc_gamma.2.weight': (512, 512), 'fc_gamma.2.bias': (512,), 'w_qs.weight': (512, 512),
              'w_ks.weight': (512, 512), 'w_vs.weight': (512, 512)}
    return {k: (torch.randn(*s, generator=g, dtype=torch.float64) / (s[-1] ** 0.5 if len(s) == 2 else 4.0))
            for k, s in shapes.items()}


@pytest.mark.parametrize('B,n,dp,gain', [(2, 37, 64, 1.0), (1, 20, 32, 256.0), (2, 5, 16, 1.0)])
def test_restatements_compose_to_the_oracle_block(B, n, dp, gain):
    p = _state(dp, 3)
    p['fc_gamma.2.weight'] *= gain
    p['fc_gamma.2.bias'] *= gain
    g = torch.Generator().manual_seed(n)
    xyz = torch.rand(B, n, 3, generator=g, dtype=torch.float64)          # continuous: tie-free distances
    feat = torch.randn(B, n, dp, generator=g, dtype=torch.float64)
    k = min(16, n)
    ref = O.transformer_block({'t.' + a: b for a, b in p.items()}, 't.', xyz, feat, k=16)
    d = O.sqdist_direct(xyz, xyz)
    sd = d.sort(dim=-1)[0]
    assert float((sd[..., 1:] - sd[..., :-1]).min()) > 0, 'tie in the distances: the argsort would be ambiguous'
    nbr = d.argsort()[:, :, :k].to(torch.int32)
    got, mid = C.block_forward(p, xyz, feat, nbr)
    assert C.rel_l2(got, ref) <= 1e-12, C.rel_l2(got, ref)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    if gain > 1:
        assert float(mid['attn'].max()) > 0.5, 'the gain should have left the near-uniform regime'


@pytest.mark.parametrize('B,n,k', C.SHAPES)
def test_logit_regimes_deliver_their_softmax_ranges(B, n, k):
    delta, vf, g = C.attn_inputs(B, n, k)
    nbr = C.neighbours('random', B, n, k)[1]
    for regime in C.REGIMES:
        L = C.logits(regime, B, n, k)
        assert L.shape == (B, n, k, 512)
        assert torch.equal(L.half().float(), L) or regime in ('uniform', 'peaked')
        mixed, mx, sm, a = C.attn(L, delta, vf, nbr)
        lo, hi = float(a.min()), float(a.max())
        if regime == 'uniform':                      # |L / sqrt(d)| < 0.1: weights within 20 % of 1 / k
            assert float((L * C.SCALE).abs().max()) < 0.1 and 0.8 / k <= lo and hi <= 1.25 / k, (lo, hi)
        elif regime == 'peaked' and k >= 4:
            spread = (L.double() * C.SCALE).amax(2) - (L.double() * C.SCALE).amin(2)
            assert float(spread.median()) > 5.0 and hi > 0.99 and lo < 1e-6, (float(spread.median()), lo, hi)
        elif regime == 'saturated':                  # exactly one-hot, in fp64 already
            assert hi == 1.0 and (lo == 0.0 or k == 1)
            assert torch.equal(a.sum(2), torch.ones_like(a.sum(2))) and bool(((a == 0) | (a == 1)).all())
            if k > 1:
                top = L.topk(2, dim=2)[0]
                assert float((top[:, :, 0] - top[:, :, 1]).min()) >= 2e4
        elif regime in ('equal_pos', 'equal_neg'):   # exactly uniform, |L| = 3e4
            assert float(L.abs().min()) == 3e4 and lo == hi == 1.0 / k
            y = C.gather(vf.double(), nbr) + delta.double()
            assert C.rel_l2(mixed, y.mean(2)) < 1e-14
        if k == 1:                                   # (e): the weight is exactly 1 whatever the logits
            assert lo == hi == 1.0
            dL = C.attn_grads(g, L, delta, vf, nbr)[0]
            assert float(dL.abs().max()) == 0.0


@pytest.mark.parametrize('B,n,k', C.SHAPES)
def test_neighbour_lists_deliver_what_they_promise(B, n, k):
    for kind in C.LIST_KINDS:
        xyz, nbr = C.neighbours(kind, B, n, k)
        assert nbr.shape == (B, n, k) and nbr.dtype == torch.int32 and xyz.shape == (B, n, 3)
        assert int(nbr.min()) >= 0 and int(nbr.max()) < n
        off, ent = C.reverse_lists(nbr)
        assert off.shape == (B, n + 1) and bool((off[:, 0] == 0).all()) and bool((off[:, -1] == n * k).all())
        flat = nbr.numpy().reshape(B, n * k)
        for b in range(B):
            for m in range(n):
                lst = ent[b, off[b, m]:off[b, m + 1]]
                assert bool((flat[b, lst] == m).all()) and bool((np.diff(lst) > 0).all())
        lens = np.diff(off, axis=1)
        if kind == 'knn':
            assert bool((nbr[:, :, 0] == torch.arange(n, dtype=torch.int32)).all()), 'self first'
            d = ((xyz.double()[:, :, None] - xyz.double()[:, None]) ** 2).sum(-1)
            kth = d.gather(2, nbr.long()).amax(2)
            assert bool(((d <= kth[:, :, None]).sum(2) == k).all()), 'the k nearest, no more'
        if kind == 'random' and k >= 4 and n <= 64:
            assert any(len(set(r.tolist())) < k for r in nbr.reshape(-1, k)), 'repeats inside a row'
        if kind == 'hub':
            assert int(lens[:, 0].min()) >= n, 'the hub is named by every point'
            assert int((lens == 0).sum(1).min()) >= n // 2 and bool((lens[:, C.orphans(n)] == 0).all())
        if kind == 'padded' and n // 3:
            assert bool((xyz[:, n - n // 3:] == xyz[:, :1]).all())
            if n // 3 + 1 > k:      # more coincident points than a list holds: the later copies' lists miss themselves
                own = (nbr == torch.arange(n, dtype=torch.int32)[None, :, None]).any(2)
                assert not bool(own.all())


def test_dyadic_pos1_inputs_are_exact_in_fp32():
    """The backward case of pos1: W1 . rel + b1 has the same value (and sign) in fp32 as in fp64."""
    xyz, nbr = C.neighbours('random', 2, 37, 15)
    xyz = C.dyadic_xyz(xyz)
    w1, b1 = C.pos1_inputs(2, 37, True)
    rel = xyz[:, :, None] - C.gather(xyz, nbr)
    pre32 = (rel[..., None, :] * w1).sum(-1) + b1
    pre64 = rel.double() @ w1.double().t() + b1.double()
    assert torch.equal(pre32.double(), pre64)
