"""GPU: the EdgeConv backwards at B = 2, N = 2048, k = 20, Co = 64 -- 40 960 entries per cloud, the size the LDS-resident
reverse-list build refuses and sug_knn_reverse now hands to the tiled build -- against the fp64 restatements of
tests/edgeconv_large_cases.py under the project's bound: per tensor err(kernel) <= 8 err(fp32 torch) + 1e-7;
each tensor's two figures are printed as `edgeconv-large-ratio <test> <tensor> ...` before the assertion.  Every backward
runs twice and gives the same bits.  DGCNNPartSeg takes one SegStep step at N = 2048, twice from one seed."""
import hashlib

import pytest
import torch

import dgcnn_seg_cases as D
import edgeconv_large_cases as E
import reverse_lists_cases as L0
import reverse_tiled_cases as C
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu


def _bound(test, got, r64, r32):
    errs = {k: (D.err(got[k], r64[k]), D.err(r32[k], r64[k])) for k in got}
    for k, (ek, e32) in errs.items():
        print('edgeconv-large-ratio %s %s %.4g %.4g' % (test, k, ek, e32))
    for k in errs:
        assert tuple(got[k].shape) == tuple(r64[k].shape) and bool(torch.isfinite(got[k]).all()), k
    bad = {k: v for k, v in errs.items() if not D.within(*v)}
    assert not bad, '%s: err(kernel), err(fp32 torch) = %r' % (test, bad)


# ----------------------------------------------------------------------------- the lists
def test_knn_reverse_at_n2048_k20_equals_the_stable_argsort():
    from sug_amd import ops
    idx = E.inputs()['idx']
    assert L0.lds_bytes(E.B, E.N * E.K, E.N)[0] > L0.LDS_LIMIT           # the LDS build refuses this shape
    off, ent = ops.knn_reverse(idx.to(torch.int32).cuda())
    want_off, want_ent = C.reference(idx.reshape(E.B, -1), E.N)
    assert tuple(ent.shape) == (E.B, E.N * E.K)
    assert torch.equal(off.cpu().long(), want_off) and torch.equal(ent.cpu().long(), want_ent)     # every entry is valid


def test_knn_reverse_at_the_headline_shape_is_unchanged():
    from sug_amd import ops
    B, E_, N, k = L0.SHAPES['bench']
    assert L0.lds_bytes(B, E_, N)[0] <= L0.LDS_LIMIT                    # through the LDS kernel
    idx = L0.make('bench-uniform')
    off, ent = ops.knn_reverse(idx.reshape(B, N, k).cuda())
    want_off, want_ent = L0.reference('bench-uniform')
    assert torch.equal(off.cpu().long(), want_off) and torch.equal(ent.cpu().long(), want_ent)
    off2, ent2 = ops.reverse_lists(idx.cuda(), N)
    assert torch.equal(off, off2) and torch.equal(ent, ent2)


# ----------------------------------------------------------------------------- one layer
def _run_layer():
    from sug_amd import ops
    c = E.inputs()
    q = c['layer']
    leaf = lambda t: t.detach().clone().cuda().requires_grad_(True)
    x, W, gamma, beta = leaf(c['x'].transpose(1, 2).contiguous()), leaf(q['W']), leaf(q['gamma']), leaf(q['beta'])
    rm, rv = q['mean'].clone().cuda(), q['var'].clone().cuda()
    pq = ops.linear_rows(x, ops.edge_weight_split(W))
    out, _ = ops.edgeconv_bn_act_max(pq, c['idx'].to(torch.int32).cuda(), gamma, beta, rm, rv, True, E.SLOPE, eps=D.EPS,
                                     momentum=D.MOMENTUM)
    out.backward(E.probes()[0].transpose(1, 2).contiguous().cuda())
    torch.cuda.synchronize()
    return {'out': out.detach().transpose(1, 2).cpu(), 'dx': x.grad.transpose(1, 2).cpu(), 'dW': W.grad.cpu(),
            'dgamma': gamma.grad.cpu(), 'dbeta': beta.grad.cpu(), 'mean': rm.cpu(), 'var': rv.cpu()}


def test_edgeconv_layer_against_fp64_and_twice_the_same_bits():
    got = _run_layer()
    _bound('layer', got, E.layer_reference('float64'), E.layer_reference('float32'))
    again = _run_layer()
    for k_ in got:
        assert torch.equal(got[k_], again[k_]), k_


# ----------------------------------------------------------------------------- the two-layer block
def _bn_module(Cn, p, i):
    bn = torch.nn.BatchNorm2d(Cn, eps=D.EPS, momentum=D.MOMENTUM).cuda().train(True)
    with torch.no_grad():
        bn.weight.copy_(p['gamma' + i]), bn.bias.copy_(p['beta' + i]), bn.running_mean.copy_(p['mean' + i]), bn.running_var.copy_(p['var' + i])
    return bn


def _run_block(fused):
    from sug_amd import ops
    c = E.inputs()
    p = c['p']
    leaf = lambda t: t.detach().clone().cuda().requires_grad_(True)
    x, W1, W2 = leaf(c['x'].transpose(1, 2).contiguous()), leaf(p['W1']), leaf(p['W2'])
    bn1, bn2 = _bn_module(D.C1, p, '1'), _bn_module(E.CO, p, '2')
    keep, ops.EDGE2_FUSED = ops.EDGE2_FUSED, fused
    try:
        assert ops.edgeconv2_supported(E.K, D.C1, E.CO) == fused
        pq = ops.linear_rows(x, ops.edge_weight_split(W1))
        out = ops.edgeconv2(pq, c['idx'].to(torch.int32).cuda(), bn1, p['slope1'], W2, None, bn2, p['slope2'])
        out.backward(E.probes()[1].transpose(1, 2).contiguous().cuda())
    finally:
        ops.EDGE2_FUSED = keep
    torch.cuda.synchronize()
    return {'out': out.detach().transpose(1, 2).cpu(), 'dx': x.grad.transpose(1, 2).cpu(), 'dW1': W1.grad.cpu(), 'dW2': W2.grad.cpu(),
            'dgamma1': bn1.weight.grad.cpu(), 'dbeta1': bn1.bias.grad.cpu(), 'dgamma2': bn2.weight.grad.cpu(),
            'dbeta2': bn2.bias.grad.cpu(), 'mean1': bn1.running_mean.cpu(), 'var1': bn1.running_var.cpu(),
            'mean2': bn2.running_mean.cpu(), 'var2': bn2.running_var.cpu()}


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_edgeconv2_against_fp64_and_twice_the_same_bits(fused):
    assert E.inputs()['p']['b1'] is None and E.inputs()['p']['b2'] is None
    got = _run_block(fused)
    _bound('edgeconv2-' + ('fused' if fused else 'composed'), got, E.block_reference('float64'), E.block_reference('float32'))
    again = _run_block(fused)
    for k_ in got:
        assert torch.equal(got[k_], again[k_]), k_


# ----------------------------------------------------------------------------- the network
def _one_step():
    from sug_amd.model.dgcnn_seg import DGCNNPartSeg
    from sug_amd.seg_step import SegStep
    m = D.MODEL
    net = D.build_model(DGCNNPartSeg, dropout=0.5).cuda().train()
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    step = SegStep(net, lr=1e-3)
    step.set_epoch(1, 10)
    g = torch.Generator().manual_seed(17)
    pts = O.synth_clouds(E.B, E.N, g).squeeze(-1).contiguous()                           # [B,3,N]
    cat = torch.tensor([3, 10])
    lab = torch.stack([D.PART_FIRST[c] + torch.randint(0, D.PART_COUNT[c], (E.N,), generator=g) for c in cat.tolist()])
    assert m['k'] == E.K and tuple(pts.shape) == (E.B, 3, E.N)
    loss = float(step.step(pts.cuda(), cat.cuda(), lab.cuda()))
    h = hashlib.sha256()
    for p in net.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    return loss, h.hexdigest()


def test_dgcnn_part_seg_takes_a_step_at_n2048_reproducibly():
    a, b = _one_step(), _one_step()
    assert a[0] == a[0] and abs(a[0]) < float('inf'), a[0]
    assert a == b
