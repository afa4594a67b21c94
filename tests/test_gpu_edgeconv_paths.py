"""GPU: the single EdgeConv layer on every dispatch path (tests/edgeconv_paths_cases.py: the fused layer with CIN = 4 / 64 /
128, Q in LDS and parked in the z buffer; the LDS-resident forward and backward with psplit 4 and 1, two passes over the
points, the XCD remap under groups; the generic kernels <1>, <2>, <4> with nch = 3 and 4, k = 7 / 20 / 255, N past the LDS
forward; train and eval mode on each) through the entry a model takes -- conv_2d.edge_rows for the fused cases,
ops.linear_rows + ops.edgeconv_bn_act_max for the others -- against the fp64 restatement under the project's bound
(DESIGN 4b): per tensor err(kernel) <= 8 err(fp32 torch) + 1e-7.  Each tensor's two figures are printed as
`edgeconv-paths-ratio <case> <tensor> <err kernel> <err fp32>` before the assertion (profiles/edgeconv_paths_fp64_ratios.txt).
Every case runs twice and gives the same bits; before it runs, the path it takes is asserted from the library's answers."""
import pytest
import torch

import dgcnn_seg_cases as D
import edgeconv_paths_cases as P

pytestmark = pytest.mark.gpu

RUNS = [(n, False) for n in P.CASES] + [('lds-psplit4', True)]          # True: SUG_EDGECONV_BWD_LEGACY=1 for the case


def _rows(t):
    return t.transpose(1, 2).contiguous()


def _assert_path(name, legacy):
    from sug_amd import ops
    s, e = P.shape(name), P.EXPECT[name]
    B, N, k, C, Co, G = s['B'], s['N'], s['k'], s['C'], s['Co'], s['G']
    assert bool(ops.edgeconv_fused_supported(N, k, C, Co)) == e['fused'], name
    if not e['fused']:
        assert ops.edgeconv_path(False, B if s['train'] else B // G, N, k, Co) == (e['fwd'] == 'lds'), name
    assert ops.edgeconv_path(True, B, N, k, Co) == (e['bwd'] == 'lds' and not legacy), name


def _run(name, legacy=False):
    """One forward + backward of the case on the device -> the compared tensors on the CPU, in the restatement's layout."""
    from sug_amd import ops
    from sug_amd.model.model_utils import conv_2d
    c, e = P.inputs(name), P.EXPECT[name]
    B, N, C, Co, G, train = c['B'], c['N'], c['C'], c['Co'], c['G'], c['train']
    leaf = lambda t: t.detach().clone().cuda().requires_grad_(True)
    x = leaf(_rows(c['x']))
    idx = c['idx'].to(torch.int32).cuda()
    gout = _rows(P.probe(name)[0]).cuda()
    keep = ops.EDGECONV_FUSED, ops.EDGECONV_FUSED_MAXC
    try:
        if e['fused']:
            ops.EDGECONV_FUSED, ops.EDGECONV_FUSED_MAXC = True, 128 if e.get('maxc') else 64
        _assert_path(name, legacy)
        if e['fused']:
            m = conv_2d(2 * C, Co, 1, activation='leakyrelu', bias=c['bias'])
            with torch.no_grad():
                m.conv[0].weight.copy_(c['W'].view(Co, 2 * C, 1, 1))
                if c['bias']:
                    m.conv[0].bias.copy_(c['b'])
                bn = m.conv[1]
                bn.weight.copy_(c['gamma']), bn.bias.copy_(c['beta']), bn.running_mean.copy_(c['mean']), bn.running_var.copy_(c['var'])
            assert bn.eps == D.EPS and bn.momentum == D.MOMENTUM
            m = m.cuda().train(train)
            with ops.bn_groups(G):
                out = m.edge_rows(x, idx)
            out.backward(gout)
            bn = m.conv[1]
            assert int(bn.num_batches_tracked) == (G if train else 0)
            Wg, bg = m.conv[0].weight.grad.view(Co, 2 * C), m.conv[0].bias.grad if c['bias'] else None
            gg, gb, rm, rv = bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var
        else:
            W, gamma, beta = leaf(c['W']), leaf(c['gamma']), leaf(c['beta'])
            b = leaf(c['b']) if c['bias'] else None
            rm, rv = c['mean'].clone().cuda(), c['var'].clone().cuda()
            pq = ops.linear_rows(x, ops.edge_weight_split(W))
            if b is not None:                                                   # the bias rides on the Q half
                pq = pq + torch.cat((torch.zeros_like(b), b))
            assert tuple(pq.shape) == (B, N, 2 * Co) and pq.data_ptr() % 16 == 0
            with ops.bn_groups(G):
                out, _ = ops.edgeconv_bn_act_max(pq, idx, gamma, beta, rm, rv, train, c['slope'], eps=D.EPS, momentum=D.MOMENTUM)
            out.backward(gout)
            Wg, bg, gg, gb = W.grad, None if b is None else b.grad, gamma.grad, beta.grad
        assert idx.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    finally:
        ops.EDGECONV_FUSED, ops.EDGECONV_FUSED_MAXC = keep
    torch.cuda.synchronize()
    got = {'out': _rows(out.detach()).cpu(), 'dx': _rows(x.grad).cpu(), 'dW': Wg.cpu(), 'dgamma': gg.cpu(), 'dbeta': gb.cpu(),
           'mean': rm.detach().cpu().clone(), 'var': rv.detach().cpu().clone()}
    if bg is not None:
        got['db'] = bg.cpu()
    return got


def _bound(label, name, got):
    r64, r32 = P.reference(name, 'float64'), P.reference(name, 'float32')
    errs = {t: (D.err(got[t], r64[t]), D.err(r32[t], r64[t])) for t in P.compared(name)}
    for t, (ek, e32) in errs.items():
        print('edgeconv-paths-ratio %s %s %.4g %.4g' % (label, t, ek, e32))
    for t in errs:
        assert tuple(got[t].shape) == tuple(r64[t].shape) and bool(torch.isfinite(got[t]).all()), (label, t)
    bad = {t: v for t, v in errs.items() if not D.within(*v)}
    assert not bad, '%s: err(kernel), err(fp32 torch) = %r' % (label, bad)
    return errs


@pytest.mark.parametrize('name,legacy', RUNS, ids=[n + ('+legacy' if l else '') for n, l in RUNS])
def test_edgeconv_layer_path_against_fp64_and_twice_the_same_bits(name, legacy, monkeypatch):
    monkeypatch.delenv('SUG_EDGECONV_BWD_LEGACY', raising=False)
    c = P.inputs(name)
    lds = _run(name) if legacy else None               # the LDS backward's result, before the switch
    if legacy:                                         # edgeconv.hip reads it with getenv at every call
        monkeypatch.setenv('SUG_EDGECONV_BWD_LEGACY', '1')
    got = _run(name, legacy)
    errs = _bound(name + ('+legacy' if legacy else ''), name, got)
    if c['train'] and c['bias']:
        # a conv bias in front of train-mode BatchNorm has zero gradient: rounding noise only
        assert float(got['db'].abs().max()) <= 1e-3 * float(got['dW'].abs().max()) + 1e-5
    if not c['train']:                                 # eval mode leaves the running buffers alone
        assert torch.equal(got['mean'], c['mean']) and torch.equal(got['var'], c['var'])
    if legacy:
        # the generic <1,20> scatter on a shape the LDS kernel normally takes: another summation order, the same gradient
        ref = P.reference(name, 'float64')['dx']
        diff = float((got['dx'].double() - lds['dx'].double()).abs().max() / float(ref.abs().max()))
        print('edgeconv-paths-legacy-vs-lds %s dx %.4g' % (name, diff))
        assert D.within(diff, errs['dx'][1])
        for t in ('out', 'mean', 'var', 'dgamma', 'dbeta'):        # nothing in front of the scatter depends on the switch
            assert torch.equal(got[t], lds[t]), t
    again = _run(name, legacy)
    assert set(again) == set(got)
    for t in got:
        assert torch.equal(got[t], again[t]), (name, t)
