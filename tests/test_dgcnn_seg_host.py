"""Host: the C ABI declares the two-layer EdgeConv block, and the restatements of tests/dgcnn_seg_cases.py are trusted
before tests/test_gpu_edgemlp.py and tests/test_gpu_dgcnn_seg.py compare the GPU with them: gradcheck of the block in fp64,
the block against the naive torch.nn composition, the split form of the head against the concatenated one, and the share of
(point, channel) pairs every block case leaves out of its probe."""
import os
import re

import pytest
import torch

import dgcnn_seg_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('sug_edgemlp_supported', 'sug_edge_expand_fwd', 'sug_edgemlp_max_layer_fwd_xf', 'sug_edge_expand_bwd')


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    from sug_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.DECLARATIONS, name
    assert _lib.CONSTANTS['SUG_ABI_VERSION'] == 8
    text = open(os.path.join(ROOT, 'include', 'sug_amd.h')).read()
    assert re.search(r'#define\s+SUG_ABI_VERSION\s+8\b', text)
    # the short-segment layer takes the arguments of its long-segment sibling
    assert _lib.DECLARATIONS['sug_edgemlp_max_layer_fwd_xf'] == _lib.DECLARATIONS['sug_pointmlp_max_layer_fwd_xf']
    src = open(os.path.join(ROOT, 'sug_amd', 'csrc', 'edgemlp.hip')).read()
    for name in ENTRY_POINTS:
        assert re.search(r'extern "C" int %s\(' % name, src), name


def test_python_side_exists():
    from sug_amd import ops
    from sug_amd.model.dgcnn_seg import DGCNNPartSeg
    from sug_amd.model.model_utils import transform_net
    assert callable(ops.edgeconv2) and callable(ops.edgeconv2_supported)
    assert hasattr(transform_net, 'edge_rows')
    net = DGCNNPartSeg(emb_dims=64)
    assert DGCNNPartSeg.graph_capturable is False
    for i in range(1, 12):
        assert hasattr(net, 'conv%d' % i)
    assert net.conv8[0].weight.shape == (256, 64 + 64 + 192, 1) and net.conv11.bias is None
    assert net.conv1[1] is net.bn1 and net.conv10[1] is net.bn10
    assert not bool(net.transform_net.fc3.weight.any()) and not bool(net.transform_net.fc3.bias.any())   # starts as the identity
    with pytest.raises(RuntimeError, match='HIP device'):
        net(torch.zeros(2, 3, 64), torch.zeros(2, dtype=torch.int64))


def _small(train_seed):
    g = D.gen('host-small', train_seed)
    B, N, k, Co = 2, 9, 4, 64
    x = torch.randn(B, 3, N, generator=g, dtype=torch.float64)
    idx, _, _ = D.lists(B, N, k, g)
    return x, idx, D._cast(D._params(Co, g), torch.float64)


@pytest.mark.parametrize('train', [True, False])
def test_gradcheck_of_the_block_restatement(train):
    x, idx, p = _small(int(train))
    nstar = D.block(x, p, idx, train)['nstar']            # the routing is piecewise constant: fixed for the finite differences
    names = [n for n in D.GRAD_NAMES[1:] if p[n] is not None]

    def f(x_, *ts):
        q = dict(p)
        q.update(zip(names, ts))
        return D.block(x_, q, idx, train, nstar)['out']

    leaves = [x.clone().requires_grad_(True)] + [p[n].clone().requires_grad_(True) for n in names]
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize('name', ['multi', 'k2'])
@pytest.mark.parametrize('train', [True, False])
def test_block_restatement_equals_the_naive_composition(name, train):
    c = D.block_case(name)
    p = D._cast(c['p'], torch.float64)
    r = D.block(c['x'].double(), p, c['idx'], train)
    out, b1, b2 = D.naive_block(c['x'].double(), p, c['idx'], train)
    # the gather at the extreme of the pre-BatchNorm y2 IS the max of the activations (monotone per channel)
    assert D.err(r['out'], out.detach()) <= 1e-13
    for bn, i in ((b1, '1'), (b2, '2')):
        assert D.err(r['mean' + i], bn.running_mean) <= 1e-13 and D.err(r['var' + i], bn.running_var) <= 1e-13


def test_head_split_equals_concat():
    g_ = D.gen('head')
    B, N, emb = 3, 17, 40
    W8 = torch.randn(256, emb + 64 + 192, generator=g_, dtype=torch.float64)
    g, l = torch.randn(B, emb, generator=g_, dtype=torch.float64), torch.randn(B, 64, generator=g_, dtype=torch.float64)
    feats = torch.randn(B, N, 192, generator=g_, dtype=torch.float64)
    a, b = D.head_split(W8, g, l, feats), D.head_concat(W8, g, l, feats)
    assert a.shape == b.shape == (B, N, 256)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


@pytest.mark.parametrize('name', list(D.SHAPES))
def test_block_cases_keep_the_cap(name):
    c = D.block_case(name)
    B, N, k = c['B'], c['N'], c['k']
    idx = c['idx']
    assert not bool((idx == N - 1).any()), 'a point named by no list'
    assert bool((idx == D.HUB).any(dim=2).all()), 'a point named by every list'
    i = torch.arange(N)
    assert bool((idx[:, i, c['j1']] == D.HUB).all()) and bool((idx[:, :, c['j2']] == D.HUB).all()) and bool((c['j1'] < c['j2']).all())
    assert any(int(torch.unique(row).numel()) < k for row in idx.reshape(-1, k)[:50]) or k == 2       # repeats
    for m in D.MODES:
        print('dgcnn-seg-zeroed %s %s %.5f (draw %d)' % (name, m, c['zeroed_' + m], c['attempt']))
        assert c['zeroed_' + m] <= D.MAX_ZEROED
        r = D.block_reference(name, m, 'float64')
        won = r['nstar'] == c['j1'].view(1, 1, N)
        assert float(won.double().mean()) >= 0.05, 'the dominant row wins a share of the channels'
        assert not bool((r['nstar'] == c['j2']).any()) or k == 2, 'the restatement never routes to the copy'
    for fam in ('grid', 'gauss'):
        kc = D.kernel_case(name, fam)
        r = D.kernel_reference(kc, torch.float64)
        if fam == 'grid':       # every value is exact in fp32
            for t in ('y1', 'a1', 'y2', 'zext', 'out'):
                assert torch.equal(r[t].float().double(), r[t]), t
            r32 = D.kernel_reference(kc, torch.float32)
            assert torch.equal(r32['nstar'], r['nstar']) and torch.equal(r32['out'].double(), r['out'])
        else:
            assert float((r['gap'] < D.TAU_GAP * r['rms']).double().mean()) <= D.MAX_ZEROED
