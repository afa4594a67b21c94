"""Class counts other than ten on the GPU: the SDA-weights kernel for 2 <= C <= 64, the MMD terms, the fused heads' last
layer for 32 < C <= 64, the step drivers, eval_worker and the loader -- against the fp64 restatement of
tests/num_class_cases.py (pinned at C = 10 against the oracle in tests/test_num_class_host.py) with the tolerances of the
ten-class tests (tests/test_gpu_mmd.py, tests/test_gpu_heads.py, tests/test_gpu_class_mmd.py).

The fp32 CPU evaluation of the restatement stays within 0.07 of the SDA tolerance at every case ("Other class
counts"), so every count keeps rtol 2e-4, atol 1e-7."""
import json
import os
import subprocess
import sys

import pytest
import torch

import num_class_cases as NC
from conftest import ROOT
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-5)                     # tests/test_gpu_mmd.py
DEV = 'cuda'


def _cuda(ts):
    return [t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------------ 1. SDA weights
@pytest.mark.parametrize('m', NC.SDA_ROWS)
@pytest.mark.parametrize('C', NC.SDA_COUNTS)
def test_sda_weights_kernel_against_fp64(C, m):
    """ops.sda_prob_weights and prob_weights_soft(num_class=C), the four weightings; m = 300 is more rows than threads."""
    from sug_amd import ops
    from sug_amd.model import mmd
    case = NC.sda_case(C, m)
    frac = NC.mean2one_fraction(*case, NC.LABEL_WEIGHT, C)
    assert 0.05 <= frac <= 0.95, frac
    ps, pt, ls, lt = _cuda(case)
    for meth in NC.SDA_METHODS:
        want = NC.sda_expected(C, m, meth)
        got = ops.sda_prob_weights(ps, pt, ls, lt, NC.LABEL_WEIGHT, meth)
        err = float(((got.cpu().double() - want.reshape(-1)).abs() / (1e-7 + 2e-4 * want.reshape(-1).abs())).max())
        print('sda C=%d m=%d %s: error / tolerance %.4f' % (C, m, meth, err))
        assert got.shape == (m,)
        torch.testing.assert_close(got.cpu().double(), want.reshape(-1), **NC.SDA_TOL)
        via = mmd.prob_weights_soft(ps, pt, ls, lt, NC.LABEL_WEIGHT, meth, num_class=C)
        assert via.shape == (1, m) and torch.equal(via.reshape(-1), got)


@pytest.mark.parametrize('m', NC.SDA_ROWS)
@pytest.mark.parametrize('C', NC.SDA_COUNTS)
def test_sda_weights_multi_equals_single_launches(C, m):
    """Three heads in one launch: each equals its own single launch bit for bit (as tests/test_gpu_mmd.py does at ten
    classes), and meets the fp64 restatement; one head reads rows of a wider buffer (row stride > C)."""
    from sug_amd import ops
    case = NC.sda_case(C, m)
    assert 0.05 <= NC.mean2one_fraction(*case, NC.LABEL_WEIGHT, C) <= 0.95
    ps, pt, ls, lt = _cuda(case)
    g = torch.Generator().manual_seed(7 * C + m)
    wide = torch.randn(m, C + 3, generator=g).cuda()
    heads = [(ps, pt), (pt * 0.5, ps + 0.25), (wide[:, :C], pt)]
    for meth in NC.SDA_METHODS:
        outs = ops.sda_prob_weights_multi(heads, ls, lt, NC.LABEL_WEIGHT, meth)
        assert len(outs) == 3
        for (a, b), o in zip(heads, outs):
            assert torch.equal(o, ops.sda_prob_weights(a, b, ls, lt, NC.LABEL_WEIGHT, meth))
        torch.testing.assert_close(outs[0].cpu().double(), NC.sda_expected(C, m, meth).reshape(-1), **NC.SDA_TOL)
        if meth != 'mean2one':                  # (the other heads' 1 / mean fractions are not chosen: no truncation for them)
            for (a, b), o in zip(heads[1:], outs[1:]):
                # these inputs are not chosen either: at C = 2, m = 300 a row's distance comes out near 1e-8, where
                # x log(x / y) - x + y cancels and 'naive_inverse' divides by distance + 1e-8.  The bound is therefore the
                # kernel's tolerance or 4 x what the fp32 CPU evaluation of the same lines loses, whichever is larger
                args = (a.cpu(), b.cpu(), case[2], case[3], NC.LABEL_WEIGHT, meth, C)
                want = NC.sda_weights(*args).reshape(-1)
                lost = float((NC.sda_weights(*args, dtype=torch.float32).reshape(-1).double() - want).abs().max())
                torch.testing.assert_close(o.cpu().double(), want, rtol=NC.SDA_TOL['rtol'], atol=max(NC.SDA_TOL['atol'], 4 * lost))


def test_sda_weights_range_and_the_ten_class_body():
    from sug_amd import ops
    from sug_amd.model import mmd
    g = torch.Generator().manual_seed(3)
    ls = torch.randint(0, 10, (8,), generator=g).cuda()
    for C in (65, 1):
        p = torch.randn(8, C, generator=g).cuda()
        with pytest.raises(RuntimeError, match=r'2\.\.64 classes'):
            ops.sda_prob_weights(p, p, ls % C, ls % C, 0.5, 'none')
        with pytest.raises(RuntimeError, match=r'2\.\.64 classes'):
            ops.sda_prob_weights_multi([(p, p), (p, p)], ls % C, ls % C, 0.5, 'none')
    # beyond 64 classes prob_weights_soft composes the weights from torch ops, with the same count
    ps, pt = torch.randn(8, 70, generator=g), torch.randn(8, 70, generator=g)
    l70 = torch.randint(0, 70, (8,), generator=g)
    got = mmd.prob_weights_soft(ps.cuda(), pt.cuda(), l70.cuda(), l70.cuda(), 0.5, 'none', num_class=70)
    torch.testing.assert_close(got.cpu().double(), NC.sda_weights(ps, pt, l70, l70, 0.5, 'none', 70), **NC.SDA_TOL)
    with pytest.raises(ValueError, match=r'70 .*num_class is 10'):
        mmd.prob_weights_soft(ps.cuda(), pt.cuda(), l70.cuda(), l70.cuda(), 0.5, 'none')
    # ten classes: the same launch as before, run to run bit for bit, and the oracle's numbers
    ps, pt = torch.randn(300, 10, generator=g) * 2, torch.randn(300, 10, generator=g) * 2
    l1, l2 = torch.randint(0, 10, (300,), generator=g), torch.randint(0, 10, (300,), generator=g)
    for meth in ('none', 'exp_inverse'):
        a = ops.sda_prob_weights(ps.cuda(), pt.cuda(), l1.cuda(), l2.cuda(), 0.5, meth)
        b = ops.sda_prob_weights(ps.cuda(), pt.cuda(), l1.cuda(), l2.cuda(), 0.5, meth)
        assert torch.equal(a, b)
        torch.testing.assert_close(a.cpu(), O.prob_weights_soft(ps, pt, l1, l2, 0.5, meth).reshape(-1), **NC.SDA_TOL)
    # a label outside [0, C): no one-hot entry, nothing raised (the rule of the ten-class kernel)
    case = NC.sda_case(11, 5)
    ps, pt, ls, lt = _cuda(case)
    bad = ls.clone()
    bad[2] = 11
    got = ops.sda_prob_weights(ps, pt, bad, lt, 0.5, 'none')

    def aug(pred, lab):
        oh = torch.zeros(5, 11, dtype=torch.float64)
        for i, v in enumerate(lab.tolist()):
            if 0 <= v < 11:
                oh[i, v] = 1
        v = torch.cat((torch.softmax(pred.double(), dim=1), oh * 0.5), dim=1) + NC.EPS
        return v / v.sum()
    a, b = aug(case[0], bad.cpu()), aug(case[1], case[3])
    want = (0.5 * (a * torch.log(a / b) - a + b) + 0.5 * (b * torch.log(b / a) - b + a)).sum(1)
    torch.testing.assert_close(got.cpu().double(), want, **NC.SDA_TOL)


# ------------------------------------------------------------------------------------------------ 2. MMD terms
def _grad_close(got, want):
    s = float(want.abs().max())
    torch.testing.assert_close(got.cpu().double(), want, rtol=1e-3, atol=2e-4 * s)


def test_mmd_terms_at_eleven_classes():
    """soft_mmd, hard_mmd, max_hard_mmd(pairing='stable'), soft_mmd_multi and soft_mmd_sharded at C = 11, m = 8, D = 266:
    values within TOL of the fp64 restatement, gradients within the fp64 gradient bound of tests/test_gpu_mmd.py."""
    from sug_amd.model import mmd
    C = 11
    X, Y, ls, lt, w = NC.mmd_case(C)
    Xd, Yd = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    want = NC.soft_mmd(ls, Xd, lt, Yd, 5.0, w, C)
    want.backward()
    Xg, Yg = X.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)
    lsg, ltg, wg = ls.cuda(), lt.cuda(), w.cuda()
    v = mmd.soft_mmd(lsg, Xg, ltg, Yg, 5.0, sample_weights=wg, num_class=C)
    v.backward()
    torch.testing.assert_close(v.detach().cpu().double(), want.detach(), **TOL)
    _grad_close(Xg.grad, Xd.grad)
    _grad_close(Yg.grad, Yd.grad)
    # mmd_cal reads the count from the term's dict
    cfg = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 5, 'NUM_CLASS': C}
    assert torch.equal(mmd.mmd_cal(lsg, Xg.detach(), ltg, Yg.detach(), cfg, sample_weights=wg), v.detach())
    # sharded: the whole batch as one rank's shard
    vs = mmd.soft_mmd_sharded(lsg, Xg.detach(), ltg, Yg.detach(), lsg, Xg.detach(), ltg, Yg.detach(), 5.0, 0, sample_weights=wg,
                              world=1, num_class=C)
    torch.testing.assert_close(vs.cpu(), v.detach().cpu(), **TOL)
    # hard / stable max-overlap: class 10 pairs rows
    for fn, ref in ((lambda a, b: mmd.hard_mmd(lsg, a, ltg, b, num_class=C), lambda a, b: NC.hard_mmd(ls, a, lt, b)),
                    (lambda a, b: mmd.max_hard_mmd(lsg, a, ltg, b, pairing='stable', num_class=C),
                     lambda a, b: NC.max_hard_mmd_stable(ls, a, lt, b, C))):
        Xd, Yd = X.double().requires_grad_(True), Y.double().requires_grad_(True)
        want = ref(Xd, Yd)
        want.backward()
        Xg, Yg = X.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)
        got = fn(Xg, Yg)
        got.backward()
        torch.testing.assert_close(got.detach().cpu().double(), want.detach(), **TOL)
        _grad_close(Xg.grad, Xd.grad)
        _grad_close(Yg.grad, Yd.grad)
    assert len(mmd.class_pairs_host(ls, lt, 1, num_class=C)[0]) > len(mmd.class_pairs_host(ls, lt, 1)[0])
    ten = mmd.max_hard_mmd(lsg, X.cuda(), ltg, Y.cuda(), pairing='stable')
    assert not torch.equal(ten, mmd.max_hard_mmd(lsg, X.cuda(), ltg, Y.cuda(), pairing='stable', num_class=C))
    sorted_ = mmd.max_hard_mmd(lsg, X.cuda(), ltg, Y.cuda(), num_class=C)      # the host pairing: same rows at m = 8
    torch.testing.assert_close(sorted_.cpu().double(), NC.max_hard_mmd_stable(ls, X.double(), lt, Y.double(), C), **TOL)


def test_soft_mmd_multi_at_eleven_classes_equals_single_calls():
    from sug_amd.model import mmd
    C = 11
    X, Y, ls, lt, _ = NC.mmd_case(C)
    g = torch.Generator().manual_seed(9)
    ps, pt = torch.randn(8, C, generator=g) * 2, torch.randn(8, C, generator=g) * 2
    lsg, ltg = ls.cuda(), lt.cuda()
    geo = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 50, 'NUM_CLASS': C}
    sem = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 5, 'SEM_WEIGHTS': 'none', 'LABEL_WEIGHT': 0.5, 'NUM_CLASS': C}
    feats = [(X.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)),
             ((X[:, :64] * 0.5).cuda().requires_grad_(True), (Y[:, :64] * 0.5).cuda().requires_grad_(True)),
             ((X[:, 64:128] + 0.1).cuda().requires_grad_(True), Y[:, 64:128].cuda().requires_grad_(True))]
    terms = [(feats[0][0], feats[0][1], geo, None, None), (feats[1][0], feats[1][1], sem, ps.cuda(), pt.cuda()),
             (feats[2][0], feats[2][1], sem, (pt * 0.5).cuda(), ps.cuda())]
    vals = mmd.soft_mmd_multi(lsg, ltg, terms)
    sum(vals).backward()
    multi_grads = [(a.grad.clone(), b.grad.clone()) for a, b in feats]
    for a, b in feats:
        a.grad = b.grad = None
    singles = [mmd.mmd_cal(lsg, fs, ltg, ft, args, data_s=ds, data_t=dt) for fs, ft, args, ds, dt in terms]
    sum(singles).backward()
    for v, s, (a, b), (ga, gb) in zip(vals, singles, feats, multi_grads):
        assert torch.equal(v, s) and torch.equal(a.grad, ga) and torch.equal(b.grad, gb)
    w1 = NC.sda_weights(ps, pt, ls, lt, 0.5, 'none', C)
    want = NC.soft_mmd(ls, (X[:, :64] * 0.5).double(), lt, (Y[:, :64] * 0.5).double(), 5.0, w1, C)
    torch.testing.assert_close(vals[1].detach().cpu().double(), want, **TOL)
    with pytest.raises(ValueError, match='one class count'):
        mmd.soft_mmd_multi(lsg, ltg, [terms[0], (feats[1][0], feats[1][1], dict(sem, NUM_CLASS=12), None, None)])


# ------------------------------------------------------------------------------------------------ 3. heads
def _heads(C, n=2, seed=3):
    from sug_amd.model.Model import Pointnet_c
    torch.manual_seed(seed)
    hs = []
    for _ in range(n):
        h = Pointnet_c(num_class=C, dgcnn_flag=True)
        for m in h.modules():                      # LayerNorm weights away from their (1, 0) initialisation
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.uniform_(-0.3, 0.3)
        h.dropout1.p = h.dropout2.p = 0.0
        hs.append(h.cuda().train())
    return hs


def _close(a, b, what):
    """tests/test_gpu_heads.py: within 2e-5 of the output / gradient scale."""
    a, b = a.detach(), b.detach()
    scale = float(b.abs().max()) + 1e-12
    err = float((a - b).abs().max()) / scale
    assert err <= 2e-5, (what, err)


def _head_grads(hs, x, outs, probe):
    loss = sum((o * p).sum() for pair, pp in zip(outs, probe) for o, p in zip(pair, pp))
    return torch.autograd.grad(loss, [x] + [p for h in hs for p in h.parameters()])


@pytest.mark.parametrize('C', [32, 40, 64])
def test_fused_heads_last_layer_up_to_64_classes(C):
    """Pointnet_c(num_class=C), M = 8, train mode with dropout 0: the fused heads (the 64-wide backward instantiation for
    C = 40 and 64) against the module path, logits, mid features and every gradient."""
    from sug_amd import ops
    hs = _heads(C)
    M = 8
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(M, 1024, generator=g) * 0.7).cuda().requires_grad_(True)
    probe = [(torch.randn(M, C, generator=g).cuda(), torch.randn(M, 256, generator=g).cuda() * 0.1) for _ in hs]
    assert ops.heads_fused_supported(hs, x)
    got = ops.heads_fused(hs, x)
    want = [h(x, adapt=True) for h in hs]
    for (gl, gm), (wl, wm) in zip(got, want):
        assert gl.shape == (M, C)
        _close(gl, wl, 'logits')
        _close(gm, wm, 'mid feature')
    names = ['x'] + ['head%d.%s' % (i, n) for i, h in enumerate(hs) for n, _ in h.named_parameters()]
    for n, a, b in zip(names, _head_grads(hs, x, got, probe), _head_grads(hs, x, want, probe)):
        _close(a, b, n)
    # one head per launch, and more rows than one 32-row block
    x2 = (torch.randn(45, 1024, generator=g) * 0.7).cuda().requires_grad_(True)
    p2 = [(torch.randn(45, C, generator=g).cuda(), torch.randn(45, 256, generator=g).cuda() * 0.1)]
    got, want = ops.heads_fused(hs[:1], x2), [hs[0](x2, adapt=True)]
    for n, a, b in zip(names, _head_grads(hs[:1], x2, got, p2), _head_grads(hs[:1], x2, want, p2)):
        _close(a, b, n + ' (45 rows)')


def test_a_33_class_model_takes_the_composed_heads(monkeypatch):
    from sug_amd import ops
    from sug_amd.model.Model import Net_MDA
    hs = _heads(33)
    x = torch.zeros(8, 1024, device=DEV)
    assert not ops.heads_fused_supported(hs, x) and not ops.heads_fused_supported(_heads(42), x)
    calls = []
    real = ops.heads_fused
    monkeypatch.setattr(ops, 'heads_fused', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(2)
    feat = (torch.randn(8, 1024, generator=g) * 0.7).cuda()
    for C, fused in ((33, 0), (40, 1)):
        net = Net_MDA('Pointnet', num_class=C)
        net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 5))
        net = net.cuda().eval()
        del calls[:]
        with torch.no_grad():
            (y1, f1), (y2, f2) = net._heads(feat)                  # what every forward of the model calls
            w1, w2 = net.c1(feat, adapt=True), net.c2(feat, adapt=True)
        assert len(calls) == fused and y1.shape == y2.shape == (8, C)
        _close(y1, w1[0], 'c1 logits')
        _close(y2, w2[0], 'c2 logits')
        _close(f1, w1[1], 'c1 mid feature')


# ------------------------------------------------------------------------------------------------ 4. steps
def _net(C, name='DGCNN', wseed=5):
    from sug_amd.model.Model import Net_MDA
    net = Net_MDA(name, num_class=C)
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, wseed))
    for mod in net.modules():
        if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)):
            mod.p = 0.0
    return net.to(DEV).train()


def _batches(C, B=4, N=1024):
    g = torch.Generator().manual_seed(11)
    out = []
    for ls, lt in NC.step_labels(C, B):
        out.append([t.to(DEV) for t in (O.synth_clouds(B, N, g), ls, O.synth_clouds(B, N, g), lt)])
    return out


def _same_as_twin(e_net, g_net, e_loss, g_loss):
    """tests/test_gpu_class_mmd.py's _same_as_twin (no NaN steps here): parameters bit for bit, losses rtol 1e-6."""
    for (k, a), (_, b) in zip(e_net.state_dict().items(), g_net.state_dict().items()):
        assert torch.equal(a, b), k
    assert all(bool(torch.isfinite(p).all()) for p in g_net.parameters())
    assert bool(torch.isfinite(e_loss).all()) and bool(torch.isfinite(g_loss).all())
    torch.testing.assert_close(g_loss, e_loss, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize('C', [11, 40])
def test_sug_step_eager_and_captured_twin(C, monkeypatch):
    """SUGStep on a C-class DGCNN, the shipped SOFT_MMD terms (SEM_WEIGHTS mean2one, LABEL_WEIGHT 0.5), labels over the full
    range: one graph is captured and equals the eager twin; the first step's three losses equal the fp64 restatement from
    that step's own logits and features; at C = 40 both forms run the fused heads."""
    from sug_amd import ops
    from sug_amd.model import mmd
    from sug_amd.train_step import SUGStep
    rec, fused = [], []
    real_multi, real_heads = mmd.soft_mmd_multi, ops.heads_fused

    def spy(ls, lt, terms, **k):
        # VALUES only (detached copies), and of the eager run's first step only: a kept tensor with a grad_fn keeps its step's
        # autograd graph alive, the parameters' AccumulateGrad nodes of that stream with it, and a capture that routes
        # gradients to those breaks (sug_amd/call_graphs.py states the mechanism)
        terms = list(terms)
        if not rec:
            val = lambda t: None if t is None else t.detach().clone()
            rec.append((ls.clone(), lt.clone(), [(val(fs), val(ft), dict(args), val(ds), val(dt)) for fs, ft, args, ds, dt in terms]))
        return real_multi(ls, lt, terms, **k)
    monkeypatch.setattr(ops, 'heads_fused', lambda *a, **k: (fused.append(1), real_heads(*a, **k))[1])
    res = {}
    for use_graph in (False, True):
        monkeypatch.setattr(mmd, 'soft_mmd_multi', real_multi if use_graph else spy)
        net = _net(C)
        tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=use_graph)
        assert tr.num_class == C and tr.methods['SEM_MMD'][0]['NUM_CLASS'] == C
        torch.manual_seed(3)
        del fused[:]
        losses = torch.stack([torch.stack([v.clone() for v in tr.step(*b)]) for b in _batches(C)]).cpu()
        assert fused, 'the fused heads did not run'
        res[use_graph] = (tr, net, losses)
    g_tr = res[True][0]
    assert len(g_tr._graphs) == 1 and next(iter(g_tr._graphs.values()))['graph'] is not None
    assert ('num_class', C) in next(iter(g_tr._graphs.keys()))
    _same_as_twin(res[False][1], res[True][1], res[False][2], res[True][2])
    # the first (eager) step against fp64, from its own tensors
    ls, lt, terms = rec[0]
    ls, lt = ls.cpu(), lt.cpu()
    assert int(ls.max()) == C - 1 and len(terms) == 3 and all(t[2]['NUM_CLASS'] == C for t in terms)
    d = lambda t: t.detach().cpu().double()
    M = res[False][0].methods
    geo, sem = M['GEO_MMD'][0], M['SEM_MMD'][0]
    want_cls = 0.5 * M['SRC_LOSS_WEIGHT'] * M['CLS_WEIGHT'] * (NC.cross_entropy(d(terms[1][3]), ls) + NC.cross_entropy(d(terms[2][3]), ls))
    want_geo = M['MMD_WEIGHT'] * geo['GEO_SCALE'] * NC.soft_mmd(ls, d(terms[0][0]), lt, d(terms[0][1]), float(geo['LABEL_SCALE']), None, C)
    sems = []
    for fs, ft, _, ps, pt in terms[1:]:
        frac = NC.mean2one_fraction(ps.cpu(), pt.cpu(), ls, lt, sem['LABEL_WEIGHT'], C)
        print('C=%d: mean2one fraction of a head %.4f' % (C, frac))
        assert 0.01 <= frac <= 0.99, frac        # (the step's own logits: not chosen, only checked to be no boundary case)
        w = NC.sda_weights(ps.cpu(), pt.cpu(), ls, lt, sem['LABEL_WEIGHT'], sem['SEM_WEIGHTS'], C)
        sems.append(NC.soft_mmd(ls, d(fs), lt, d(ft), float(sem['LABEL_SCALE']), w, C))
    want_sem = 0.5 * M['MMD_WEIGHT'] * sem['SEM_SCALE'] * (sems[0] + sems[1])
    got = res[False][2][0].double()
    print('C=%d first step: got %s want %s' % (C, got.tolist(), [float(want_cls), float(want_geo), float(want_sem)]))
    torch.testing.assert_close(got, torch.stack([want_cls, want_geo, want_sem]), **TOL)


def test_uda_step_naive_mmd_at_eleven_classes():
    from sug_amd.uda_step import UDAStep
    C, res = 11, {}
    for use_graph in (False, True):
        net = _net(C)
        tr = UDAStep(net, 'naive_mmd', lr=1e-3, weight_decay=5e-5, use_graph=use_graph)
        assert tr.class_mmd['NUM_CLASS'] == C
        torch.manual_seed(3)
        losses = torch.stack([torch.stack(tr.step(*b)) for b in _batches(C)[:2]]).cpu()
        res[use_graph] = (tr, net, losses)
    tr = res[True][0]
    assert tr.stats == {'planned': 1, 'captured': 1, 'replayed': 1, 'refused': 0} and tr.why is None, (tr.stats, tr.why)
    _same_as_twin(res[False][1], res[True][1], res[False][2], res[True][2])


def test_source_step_with_fifteen_classes():
    """SourceStep and the source-only classifier already take a count: a 15-class Pointnet_cls, captured against eager, and
    the first step's loss against the fp64 cross entropy of the eager model's logits."""
    from sug_amd.model.model_pointnet import Pointnet_cls
    from sug_amd.source_step import SourceStep
    C, res = 15, {}
    g = torch.Generator().manual_seed(6)
    batches = [(O.synth_clouds(8, 1024, g).cuda(), (torch.arange(8) + 7 * i).cuda() % C) for i in range(3)]
    for use_graph in (False, True):
        net = Pointnet_cls(num_class=C)
        net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 2))
        for mod in net.modules():
            if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)):
                mod.p = 0.0
        net = net.cuda().train()
        if not use_graph:
            with torch.no_grad():
                want = NC.cross_entropy(net(batches[0][0]).cpu().double(), batches[0][1].cpu())
            net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 2))      # (the BatchNorm buffers)
        tr = SourceStep(net, lr=1e-3, weight_decay=5e-5, use_graph=use_graph)
        torch.manual_seed(3)
        res[use_graph] = (tr, net, torch.stack([tr.step(*b).clone() for b in batches]).cpu())
    assert res[True][0].stats['captured'] == 1 and res[True][0].stats['refused'] == 0, (res[True][0].stats, res[True][0].why)
    _same_as_twin(res[False][1], res[True][1], res[False][2], res[True][2])
    torch.testing.assert_close(res[False][2][0].double(), want, **TOL)


def test_eval_worker_with_eleven_classes(tmp_path):
    """The case runs in a child process, for the reason tests/test_gpu_eval_worker.py gives (the eval runners keep private
    graph pools alive)."""
    out = str(tmp_path / 'results.json')
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(ROOT, 'tests', 'num_class_cases.py'), out]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert os.path.exists(out), 'the case process ended (exit %d):\n%s' % (r.returncode, r.stderr.decode()[-3000:])
    res = json.load(open(out))
    assert res.get('eval_worker_eleven_classes', 'missing') is None, res


def test_loader_with_fifteen_classes():
    from sug_amd.data.dataloader import DeviceLoader, UnifiedPointDG
    g = torch.Generator().manual_seed(4)
    pts = torch.rand(30, 1100, 3, generator=g) * 2 - 1
    labels = torch.arange(30) % 15
    ds = UnifiedPointDG('modelnet', pts, labels, pc_input_num=1024, aug=False, class_num=15)
    assert ds.class_num == 15 and len(ds.classes()) == 15 and ds.classes()[14] == [14, 29]
    w = ds.cls_wights()
    assert len(w) == 15 and abs(sum(w) - 1.0) < 1e-6
    data, lab = next(iter(DeviceLoader(ds, batch_size=8, shuffle=False)))
    assert data.shape == (8, 3, 1024, 1) and lab.tolist() == list(range(8)) and data.is_cuda
    assert len(UnifiedPointDG('modelnet', pts, labels % 10, pc_input_num=1024, aug=False).classes()) == 10
    with pytest.raises(ValueError, match=r'label 15 .*15'):
        UnifiedPointDG('modelnet', pts, labels + 1, pc_input_num=1024, aug=False, class_num=15)
    with pytest.raises(ValueError, match=r'label 10 .*10'):
        UnifiedPointDG('modelnet', pts, labels, pc_input_num=1024, aug=False)
