"""CPU checks of tests/edgeconv_paths_cases.py: every case's lists hold a hub and an unlisted point, its probe zeroes few
pairs, the fp32 torch form keeps the margins for the chosen seed (where the probe is not zero it routes as the fp64 form
does and stands on the same side of the activation's kink), and the case reaches the kernel its name says -- by the
library's own answers (ops.edgeconv_path, ops.edgeconv_fused_supported: host-side, no launch) and by the launch arithmetic
restated in the cases module."""
import pytest
import torch

import dgcnn_seg_cases as D
import edgeconv_paths_cases as P
import reverse_lists_cases as L0

NAMES = sorted(P.CASES)


def test_the_table_is_the_one_the_paths_need():
    assert set(P.EXPECT) == set(P.CASES) and len(P.CASES) == 18
    for name in NAMES:
        s = P.shape(name)
        assert s['B'] % s['G'] == 0 and s['Co'] % 4 == 0 and s['Co'] <= 1024 and 2 <= s['k'] <= 255, name
    # every template instance and regime has a case
    assert {P.EXPECT[n].get('nch') for n in NAMES} >= {1, 2, 3, 4}
    assert {(P.EXPECT[n]['pf'], P.EXPECT[n]['pb']) for n in NAMES if 'pf' in P.EXPECT[n]} >= {(4, 4), (1, 1)}
    assert any(not P.shape(n)['train'] and P.EXPECT[n]['fused'] for n in NAMES)
    assert any(not P.shape(n)['train'] and P.EXPECT[n].get('fwd') == 'lds' for n in NAMES)
    assert any(not P.shape(n)['train'] and P.EXPECT[n].get('fwd') == 'generic' for n in NAMES)
    assert any(P.shape(n)['k'] == 255 for n in NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_lists_hold_a_hub_and_an_unlisted_point(name):
    c = P.inputs(name)
    B, N, k = c['B'], c['N'], c['k']
    idx = c['idx']
    assert tuple(idx.shape) == (B, N, k) and int(idx.min()) >= 0 and int(idx.max()) < N
    assert torch.equal(c['x'][:, :, D.HUB], D.DOMINANT * c['x'][:, :, D.HUB + 1])
    i = torch.arange(N)
    assert bool((idx[:, i, c['j1']] == D.HUB).all()) and bool((idx[:, :, c['j2']] == D.HUB).all()) and bool((c['j1'] < c['j2']).all())
    for b in range(B):
        counts = torch.bincount(idx[b].reshape(-1), minlength=N)
        assert int(counts[D.HUB]) >= 2 * N and int(counts[N - 1]) == 0, (name, b)
    assert float(c['gamma'].abs().min()) >= 0.25 and bool((c['gamma'] > 0).any()) and bool((c['gamma'] < 0).any())
    assert not torch.equal(c['mean'], torch.zeros(c['Co'])) and not torch.equal(c['var'], torch.ones(c['Co']))
    assert (c['b'] is not None) == c['bias']


@pytest.mark.parametrize('name', NAMES)
def test_probe_zeroes_few_pairs(name):
    gout, share = P.probe(name)
    assert share <= D.MAX_ZEROED, (name, share)                  # a condition on the seed, not a measurement
    assert float((gout != 0).double().mean()) >= 1 - D.MAX_ZEROED


@pytest.mark.parametrize('name', NAMES)
def test_fp32_torch_holds_the_margins_for_this_seed(name):
    r64, r32 = P.reference(name, 'float64'), P.reference(name, 'float32')
    live = P.probe(name)[0] != 0
    assert torch.equal(r64['nstar'][live], r32['nstar'][live])
    assert torch.equal(r64['pre'][live] > 0, r32['pre'][live] > 0)
    # the copy of the hub's row never wins: the winner among the two is the earlier j
    assert not bool((r64['nstar'] == P.inputs(name)['j2']).any())
    for t in P.compared(name):
        assert D.err(r32[t], r64[t]) < 1e-4, (name, t)


@pytest.mark.parametrize('name', NAMES)
def test_case_reaches_what_its_name_says(name):
    from sug_amd import ops
    s, e = P.shape(name), P.EXPECT[name]
    B, N, k, C, Co, G = s['B'], s['N'], s['k'], s['C'], s['Co'], s['G']
    keep = ops.EDGECONV_FUSED, ops.EDGECONV_FUSED_MAXC
    try:
        ops.EDGECONV_FUSED, ops.EDGECONV_FUSED_MAXC = True, 64
        assert ops.edgeconv_fused_supported(N, k, C, Co) == (e['fused'] and not e.get('maxc', False))
        ops.EDGECONV_FUSED_MAXC = 128
        assert ops.edgeconv_fused_supported(N, k, C, Co) == e['fused']
    finally:
        ops.EDGECONV_FUSED, ops.EDGECONV_FUSED_MAXC = keep
    if e['fused']:
        assert P.fused_qlds(N) == e['qlds'] and C in (3, 64, 128)
    else:
        Bf = B if s['train'] else B // G                # eval mode runs the forward group by group
        assert ops.edgeconv_path(False, Bf, N, k, Co) == (e['fwd'] == 'lds')
        if e['fwd'] == 'lds':
            assert P.lds_psplit(False, Bf, Co) == e['pf']
    assert ops.edgeconv_path(True, B, N, k, Co) == (e['bwd'] == 'lds')
    if e['bwd'] == 'lds':
        pb = P.lds_psplit(True, B, Co)
        assert pb == e['pb']
        if 'n_own' in e:
            assert P.lds_n_own(N, pb) == e['n_own'] > 256
            assert int(torch.bincount(P.inputs(name)['idx'][0].reshape(-1), minlength=N).max()) >= 255      # shares bin 0
        else:
            assert P.lds_n_own(N, pb) <= 256
    if 'nch' in e:
        assert P.generic_nch(Co) == e['nch']
    assert (B % 8 == 0) == e.get('xcd', False)


def test_path_query_edges(monkeypatch):
    """ops.edgeconv_path on both sides of each term of the two conditions."""
    from sug_amd import ops
    monkeypatch.delenv('SUG_EDGECONV_BWD_LEGACY', raising=False)
    assert ops.edgeconv_path(False, 64, 1024, 20, 64) and ops.edgeconv_path(True, 64, 1024, 20, 64)
    assert ops.edgeconv_path(False, 2, 2272, 20, 64) and not ops.edgeconv_path(False, 2, 2273, 20, 64)      # 150 KB of LDS
    assert ops.edgeconv_path(True, 2, 1094, 20, 64) and not ops.edgeconv_path(True, 2, 1095, 20, 64)        # 158 KB
    assert ops.edgeconv_path(False, 256, 64, 20, 16) and not ops.edgeconv_path(False, 257, 64, 20, 16)      # partial rows
    assert ops.edgeconv_path(True, 257, 64, 20, 16)
    for backward in (False, True):
        assert not ops.edgeconv_path(backward, 2, 64, 19, 64) and not ops.edgeconv_path(backward, 2, 64, 20, 40)
        assert not ops.edgeconv_path(backward, 0, 64, 20, 64) and not ops.edgeconv_path(backward, 2, 0, 20, 64)
    monkeypatch.setenv('SUG_EDGECONV_BWD_LEGACY', '1')          # read at every call
    assert not ops.edgeconv_path(True, 64, 1024, 20, 64) and ops.edgeconv_path(False, 64, 1024, 20, 64)
    monkeypatch.delenv('SUG_EDGECONV_BWD_LEGACY')
    assert ops.edgeconv_path(True, 64, 1024, 20, 64)


def test_special_regimes():
    from sug_amd import ops
    s = P.shape('gen-n2304')                                     # the backward's reverse lists come from the tiled build
    assert L0.lds_bytes(s['B'], s['N'] * s['k'], s['N'])[0] > L0.LDS_LIMIT
    assert ops.reverse_lists_tiled_supported(s['B'], s['N'] * s['k'], s['N'])
    s = P.shape('fused-q-global')                                # smallest N whose Q slice is parked in the z buffer
    assert not P.fused_qlds(s['N']) and P.fused_qlds(s['N'] - 1)
    for name in ('fused-q-global', 'lds-two-pass', 'gen-n2304'):
        c = P.inputs(name)
        assert int(torch.bincount(c['idx'][0].reshape(-1), minlength=c['N'])[D.HUB]) > 2 * c['N']
