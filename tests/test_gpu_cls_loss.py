"""GPU: the fused classification-loss tail of the shipped configurations (ops.cls_loss = sug_cls_loss_fwd / sug_cls_loss_bwd) and
the steps that use it.

  1. the reference-generated goldens of focal_loss;  2. the full formula against torch in fp64 on the CPU;  3. the edges (saturated
  rows, the discrepancy's kink, labels, limits);  4. books and determinism, graph capture included;  5. SUGStep with the fused tail
  against the composed fp32 step;  6. SUGStep under graph replay against its eager twin;  7. UDAStep with focal_loss.

Tolerances are those of tests/test_gpu_loss.py: a fused loss kernel -- loss rtol 2e-6, atol 1e-7, gradients rtol 1e-5, atol 1e-7;
a step -- losses within 2e-6 * max(1, |b|), gradients rtol 2e-4, atol 2e-6 * the largest gradient entry."""
import hashlib
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS_TOL = dict(rtol=2e-6, atol=1e-7)
GRAD_TOL = dict(rtol=1e-5, atol=1e-7)
WEIGHTS = [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5]           # ten unequal class weights


# ------------------------------------------------------------------------------------------------ the formula, composed
def _row_loss(z, y, alpha, gamma, reduction, ignore_index=None):
    """model_utils.focal_loss.forward on one head (alpha None: ones); alpha None and gamma 0 with an ignore label is
    nn.CrossEntropyLoss(ignore_index=...)."""
    if ignore_index is not None:
        return F.cross_entropy(z, y, ignore_index=ignore_index, reduction=reduction)
    logp = F.log_softmax(z, dim=1).gather(1, y.view(-1, 1)).view(-1)
    a = alpha.gather(0, y) if alpha is not None else torch.ones_like(logp)
    loss = a * (-(1 - torch.exp(logp)) ** gamma * logp)
    return loss.mean() if reduction == 'mean' else loss.sum()


def _composed(zs, lab, lab_t, alpha, gamma, reduction, a_s, a_t, a_d, r_s, ignore_index=None):
    """(differentiable loss, the four outputs) from torch ops on four separate logit blocks."""
    Ls = _row_loss(zs[0], lab, alpha, gamma, reduction, ignore_index) + _row_loss(zs[1], lab, alpha, gamma, reduction, ignore_index)
    zero = torch.zeros((), dtype=zs[0].dtype, device=zs[0].device)
    Lt = (_row_loss(zs[2], lab_t, alpha, gamma, reduction, ignore_index) +
          _row_loss(zs[3], lab_t, alpha, gamma, reduction, ignore_index)) if a_t else zero
    D = torch.mean(torch.abs(F.softmax(zs[2], dim=-1) - F.softmax(zs[3], dim=-1))) if a_d else zero
    loss = a_s * Ls + a_t * Lt - a_d * D
    return loss, torch.stack([loss.detach(), r_s * Ls.detach(), -a_d * D.detach(), a_t * Lt.detach()])


def _reference(zs, lab, lab_t, alpha, gamma, reduction, a_s, a_t, a_d, r_s, g=1.7, dtype=torch.float64, device='cpu', ignore_index=None):
    zs = [z.detach().to(device=device, dtype=dtype).clone().requires_grad_() for z in zs]
    al = None if alpha is None else alpha.to(device=device, dtype=dtype)
    loss, outs = _composed(zs, lab.to(device), lab_t.to(device), al, gamma, reduction, a_s, a_t, a_d, r_s, ignore_index)
    (loss * g).backward()
    return outs.cpu().double(), [(z.grad if z.grad is not None else torch.zeros_like(z)).cpu().double() for z in zs]


def _ours(zs, lab, lab_t, alpha, gamma, reduction, a_s, a_t, a_d, r_s, g=1.7, form='separate', totals=None, ignore_index=-100):
    """ops.cls_loss on device copies of the four host blocks -> (outputs [4], the four gradient blocks).  form: 'separate' (four
    tensors), 'paired' (two [Ms + Mt, C] tensors, source rows first), 'strided' / 'paired_strided' (the same as column slices of
    wider tensors: a row stride larger than C)."""
    from sug_amd import ops
    Ms, C = zs[0].shape
    pad = 6 if 'strided' in form else 0
    if form.startswith('paired'):
        blocks = [torch.cat((zs[0], zs[2])), torch.cat((zs[1], zs[3]))]
    else:
        blocks = list(zs)
    leaves = [torch.cat((b, torch.full((b.shape[0], pad), 99.0)), dim=1).to(DEV).requires_grad_() for b in blocks]
    views = [t[:, :C] for t in leaves]
    al = None if alpha is None else alpha.to(DEV)
    lt = None if lab_t is None else lab_t.to(DEV)
    if form.startswith('paired'):
        out = ops.cls_loss(views[0], views[1], None, None, lab.to(DEV), lt, al, gamma, reduction, ignore_index, a_s, a_t, a_d, r_s, totals)
    else:
        out = ops.cls_loss(views[0], views[1], views[2], views[3], lab.to(DEV), lt, al, gamma, reduction, ignore_index, a_s, a_t, a_d,
                           r_s, totals)
    assert out[0].requires_grad and not any(o.requires_grad for o in out[1:])
    (out[0] * g).backward()
    grads = [t.grad for t in leaves]
    assert all(float(gr[:, C:].abs().sum()) == 0.0 for gr in grads)            # nothing written past the C columns
    grads = [gr[:, :C] for gr in grads]
    if form.startswith('paired'):
        grads = [grads[0][:Ms], grads[1][:Ms], grads[0][Ms:], grads[1][Ms:]]
    return torch.stack([o.detach() for o in out]), grads


def _blocks(Ms, Mt, C, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    zs = [torch.randn(M, C, generator=g) * scale for M in (Ms, Ms, Mt, Mt)]
    return zs, torch.randint(0, C, (Ms,), generator=g), torch.randint(0, C, (Mt,), generator=g)


def _alpha(C, seed=5):
    return torch.rand(C, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


def _assert_close(outs, grads, ref, gref, tag):
    print('%s: outputs %s ref %s; max gradient error %.3e' % (
        tag, outs.tolist(), ref.tolist(), max(float((a.cpu().double() - b).abs().max()) for a, b in zip(grads, gref))))
    torch.testing.assert_close(outs.cpu().double(), ref, **LOSS_TOL, msg=lambda m: '%s: %s' % (tag, m))
    for i, (a, b) in enumerate(zip(grads, gref)):
        torch.testing.assert_close(a.cpu().double(), b, **GRAD_TOL, msg=lambda m: '%s block %d: %s' % (tag, i, m))


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize('tag,avg', [('uni', True), ('cls', True), ('sum', False)])
def test_reference_goldens_through_cls_loss(tag, avg):
    """focal_loss as the reference computed it (logits, labels, alpha, gamma -> loss, gradient): ys1 = ys2 = pred with a_s = 0.5 is
    the loss itself, ds1 + ds2 its gradient; the dummy target block is not read and gets exact zeros."""
    from sug_amd import ops
    G = load_golden('focal.npz')
    pred = G[tag + '_pred'].to(DEV).requires_grad_()
    dummy = torch.full((3, pred.shape[1]), float('nan'), device=DEV).requires_grad_()
    out = ops.cls_loss(pred, pred, dummy, dummy, G[tag + '_label'].to(DEV), None, G[tag + '_alpha'].to(DEV), float(G[tag + '_gamma']),
                       'mean' if avg else 'sum', a_s=0.5, a_t=0.0, a_d=0.0)
    out[0].backward()
    torch.testing.assert_close(out[0].detach().cpu(), G[tag + '_loss'], **LOSS_TOL)
    torch.testing.assert_close(pred.grad.cpu(), G[tag + '_grad'], **GRAD_TOL)
    assert float(out[2]) == 0.0 and float(out[3]) == 0.0
    assert dummy.grad is not None and float(dummy.grad.abs().sum()) == 0.0 and not torch.isnan(dummy.grad).any()


# ------------------------------------------------------------------------------------------------ 2. the formula against fp64
COEFS = [(0.0, 0.0), (0.25, 0.0), (0.25, 0.15), (0.0, 1.0)]                 # (a_t, a_d)


@pytest.mark.parametrize('Ms,Mt,C', [(32, 32, 10), (4, 4, 10), (5, 5, 7), (3, 6, 64), (1, 1, 2), (1024, 1024, 40)])
def test_cls_loss_against_fp64(Ms, Mt, C):
    """Every gamma x alpha x reduction x (a_t, a_d), in the paired and the separate form, and once as column slices of wider
    tensors: the four outputs and the four gradient blocks (upstream gradient 1.7) against the same formula composed in torch in
    fp64 on the CPU.  One set of logits (randn * 3) per shape; the fp64 reference of a combination serves both forms."""
    zs, lab, lab_t = _blocks(Ms, Mt, C, 100 * Ms + C)
    worst = 0.0
    for gamma, per_class, reduction, (a_t, a_d) in itertools.product((0.0, 1.5, 2.0), (False, True), ('mean', 'sum'), COEFS):
        if a_t and Ms != Mt and (Ms, Mt, C) == (3, 6, 64):
            continue                                                        # (3, 6, 64) runs with a_t = 0
        alpha = _alpha(C) if per_class else torch.full((C,), 1.0 / C)
        args = (alpha, gamma, reduction, 0.35, a_t, a_d, 0.5)
        ref, gref = _reference(zs, lab, lab_t, *args)
        for form in ('separate', 'paired'):
            tag = 'M=%d/%d C=%d gamma=%g alpha=%s %s a_t=%g a_d=%g %s' % (Ms, Mt, C, gamma, 'class' if per_class else 'uni', reduction,
                                                                            a_t, a_d, form)
            outs, grads = _ours(zs, lab, lab_t if a_t else None, *args, form=form)
            _assert_close(outs, grads, ref, gref, tag)
            worst = max(worst, max(float((a.cpu().double() - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads, gref)))
            if not a_t and not a_d:
                assert float(grads[2].abs().sum()) == 0.0 and float(grads[3].abs().sum()) == 0.0      # exact zeros
    print('worst gradient error over the largest entry of its block: %.3e' % worst)
    a_t = 0.0 if Ms != Mt else 0.25
    args = (_alpha(C), 2.0, 'mean', 0.35, a_t, 0.15, 0.5)
    ref, gref = _reference(zs, lab, lab_t, *args)
    for form in ('strided', 'paired_strided'):                              # row stride C + 6
        outs, grads = _ours(zs, lab, lab_t if a_t else None, *args, form=form)
        _assert_close(outs, grads, ref, gref, 'M=%d/%d C=%d %s' % (Ms, Mt, C, form))


def test_alpha_none_is_uniform_weight_one():
    zs, lab, lab_t = _blocks(5, 5, 7, 3)
    for gamma in (0.0, 2.0):
        args = (gamma, 'mean', 0.5, 0.25, 0.15, 1.0)
        ref, gref = _reference(zs, lab, lab_t, torch.ones(7), *args)
        outs, grads = _ours(zs, lab, lab_t, None, *args)
        _assert_close(outs, grads, ref, gref, 'alpha=None gamma=%g' % gamma)


# ------------------------------------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize('gamma', [0.0, 2.0])
def test_saturated_rows_stay_finite_and_close_to_fp64(gamma):
    """A logit margin of 40: p_y rounds to 1 in fp32 (row 1 of every block, right label), and the opposite, a row whose label has
    probability ~ e^-40 (row 2)."""
    zs, lab, lab_t = _blocks(4, 4, 10, 21)
    for z, y in ((zs[0], lab), (zs[1], lab), (zs[2], lab_t), (zs[3], lab_t)):
        z[1] = 0.0
        z[1, y[1]] = 40.0
        z[2] = 0.0
        z[2, (y[2] + 1) % 10] = 40.0
    args = (_alpha(10), gamma, 'mean', 0.5, 0.25, 0.15, 1.0)
    ref, gref = _reference(zs, lab, lab_t, *args)
    outs, grads = _ours(zs, lab, lab_t, *args)
    assert torch.isfinite(outs).all() and all(torch.isfinite(g).all() for g in grads)
    _assert_close(outs, grads, ref, gref, 'margin 40, gamma=%g' % gamma)


def test_equal_target_rows_have_zero_discrepancy_gradient():
    zs, lab, lab_t = _blocks(4, 4, 10, 22)
    zs[3][0] = zs[2][0]
    zs[3][2] = zs[2][2]
    outs, grads = _ours(zs, lab, None, None, 0.0, 'mean', 1.0, 0.0, 1.0, 1.0)
    for r in (0, 2):
        assert float(grads[2][r].abs().sum()) == 0.0 and float(grads[3][r].abs().sum()) == 0.0         # sign(0) = 0
    assert float(grads[2][1].abs().sum()) > 0.0
    ref, gref = _reference(zs, lab, lab_t, None, 0.0, 'mean', 1.0, 0.0, 1.0, 1.0)
    _assert_close(outs, grads, ref, gref, 'equal target rows')


@pytest.mark.parametrize('per_class', [False, True])
def test_out_of_range_labels_poison_their_row_only(per_class):
    zs, lab, lab_t = _blocks(5, 5, 10, 9)
    alpha = _alpha(10) if per_class else None
    for bad in (10, -1, -100 if per_class else 64):          # (with alpha given there is no ignore label: -100 is out of range)
        yb = lab.clone()
        yb[3] = bad
        outs, grads = _ours(zs, yb, None, alpha, 2.0 if per_class else 0.0, 'mean', 1.0, 0.0, 1.0, 1.0)
        assert torch.isnan(outs[0]) and torch.isnan(outs[1]) and not torch.isnan(outs[2])
        assert torch.isnan(grads[0][3]).all() and torch.isnan(grads[1][3]).all()
        assert not torch.isnan(grads[0][[0, 1, 2, 4]]).any() and not torch.isnan(grads[2]).any() and not torch.isnan(grads[3]).any()
        outs, grads = _ours(zs, lab, yb, alpha, 2.0 if per_class else 0.0, 'mean', 1.0, 0.25, 1.0, 1.0)      # ... in the target labels
        assert torch.isnan(outs[0]) and torch.isnan(outs[3]) and not torch.isnan(outs[1])
        assert torch.isnan(grads[2][3]).all() and not torch.isnan(grads[2][[0, 1, 2, 4]]).any() and not torch.isnan(grads[0]).any()


@pytest.mark.parametrize('ignore_index', [-100, 3])
def test_ce_mode_honours_ignore_index_as_cross_entropy_loss(ignore_index):
    """alpha None, gamma 0: nn.CrossEntropyLoss(ignore_index=...) on source and target rows (ignored rows are skipped and left
    out of the mean)."""
    zs, lab, lab_t = _blocks(16, 16, 10, 5)
    for y in (lab, lab_t):
        y[y == ignore_index] = (ignore_index + 1) % 10
    lab[[1, 7, 8]] = ignore_index
    lab_t[[0, 15]] = ignore_index
    args = (None, 0.0, 'mean', 0.5, 0.25, 0.15, 1.0)
    ref, gref = _reference(zs, lab, lab_t, *args, ignore_index=ignore_index)
    outs, grads = _ours(zs, lab, lab_t, *args, ignore_index=ignore_index)
    _assert_close(outs, grads, ref, gref, 'ignore_index=%d' % ignore_index)
    assert float(grads[0][[1, 7, 8]].abs().sum()) == 0.0 and float(grads[1][[1, 7, 8]].abs().sum()) == 0.0
    crit = nn.CrossEntropyLoss(ignore_index=ignore_index)
    want = 0.5 * (crit(zs[0].double(), lab) + crit(zs[1].double(), lab))
    outs, _ = _ours(zs, lab, None, None, 0.0, 'mean', 0.5, 0.0, 0.0, 1.0, ignore_index=ignore_index)
    torch.testing.assert_close(outs[0].cpu().double(), want, **LOSS_TOL)


def test_unsupported_arguments_are_refused_not_computed():
    from sug_amd import _lib, ops
    zs, lab, _ = _blocks(4, 4, 10, 1)
    zg = [z.to(DEV) for z in zs]
    labg = lab.to(DEV)
    assert ops.cls_loss_supported(*zg, label=labg, gamma=2.0) and ops.cls_loss_supported(*zg, label=labg, gamma=1.0)
    assert not ops.cls_loss_supported(*zg, label=labg, gamma=0.5)
    with pytest.raises(RuntimeError, match='gamma=0.5'):
        ops.cls_loss(*zg, labg, gamma=0.5)
    assert b'sug_cls_loss_fwd' in _lib.lib().sug_last_error()
    wide = torch.zeros(4, 65, device=DEV)
    assert not ops.cls_loss_supported(wide, wide, wide, wide, label=labg)
    with pytest.raises(RuntimeError, match='C=65'):
        ops.cls_loss(wide, wide, wide, wide, labg)
    assert not ops.cls_loss_supported(*zg, label=labg, a_t=0.25)                          # no target labels
    assert not ops.cls_loss_supported(*zg, label=labg, alpha=torch.ones(9, device=DEV))   # fewer than C weights
    assert not ops.cls_loss_supported(*zg, label=labg, alpha=torch.ones(10))              # alpha on the host
    assert not ops.cls_loss_supported(*[t.half() for t in zg], label=labg)
    assert not ops.cls_loss_supported(*zg, label=labg, reduction='none')


# ------------------------------------------------------------------------------------------------ 4. books and determinism
def test_books_accumulate_in_the_same_launch():
    totals = torch.zeros(4, dtype=torch.float64, device=DEV)
    want = [0.0, 0.0, 0.0, 0.0]
    zs, lab, lab_t = _blocks(5, 5, 10, 31)
    for r_s, a_d in ((0.5, 1.0), (1.0, 0.15)):
        outs, _ = _ours(zs, lab, lab_t, _alpha(10), 2.0, 'mean', 0.25, 0.25, a_d, r_s, totals=totals)
        want[0] += float(outs[1]) * 5                       # loss_total += loss_s.item() * data.size(0)
        want[1] += float(outs[2]) * 5                       # loss_adv_total += loss_adv.item() * data.size(0)
        want[2] += 5
        want[3] += 5
    assert totals.tolist() == want, (totals.tolist(), want)


def test_two_calls_are_bit_identical():
    zs, lab, lab_t = _blocks(65, 65, 10, 32)
    args = (_alpha(10), 1.5, 'mean', 0.25, 0.25, 0.15, 0.5)
    a, ga = _ours(zs, lab, lab_t, *args)
    b, gb = _ours(zs, lab, lab_t, *args)
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(ga, gb))


def test_captured_forward_and_backward_replay_the_eager_call_bit_for_bit():
    from sug_amd import ops
    zs, lab, lab_t = _blocks(32, 32, 10, 33)
    alpha, labg = _alpha(10).to(DEV), lab.to(DEV)
    args = (alpha, 2.0, 'mean', -100, 0.25, 0.25, 0.15, 0.5)
    static = [torch.zeros(32, 10, device=DEV).requires_grad_() for _ in range(4)]
    totals = torch.zeros(4, dtype=torch.float64, device=DEV)

    def run(ts, tot):
        out = ops.cls_loss(ts[0], ts[1], ts[2], ts[3], labg, labg, *args, tot)
        grads = torch.autograd.grad(out[0] * 1.7, ts)
        return torch.stack([o.detach() for o in out]), grads
    live = [z.to(DEV).requires_grad_() for z in zs]
    want, gwant = run(live, None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # (torch's recipe: one warm-up on a side stream before a capture)
        run(static, None)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got, ggot = run(static, totals)
    with torch.no_grad():
        for s, z in zip(static, zs):
            s.copy_(z.to(DEV))
    graph.replay()
    graph.replay()
    assert torch.equal(got, want) and all(torch.equal(a, b) for a, b in zip(ggot, gwant))
    assert totals.tolist() == [2 * float(want[1]) * 32, 2 * float(want[2]) * 32, 64.0, 64.0]    # the books advance per replay


# ------------------------------------------------------------------------------------------------ models
def _net(name='Pointnet', seed=9):
    from sug_amd.model.Model import Net_MDA
    net = Net_MDA(name)
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
    for m in net.modules():
        if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)):
            m.p = 0.0
    return net.to(DEV).train()


def _class_weighting():
    """CLS_LOSS: ClassWeighting of the shipped configurations: focal_loss(gamma=0, alpha=<class weights>)."""
    from sug_amd.model.model_utils import focal_loss
    c = focal_loss(alpha=list(WEIGHTS), gamma=0, num_classes=10)
    c.alpha = c.alpha.to(DEV)           # a plain attribute, not a buffer: moved by hand so that its forward copies nothing
    return c


def _focal(gamma=2):
    from sug_amd.model.model_utils import focal_loss
    c = focal_loss(gamma=gamma, num_classes=10)
    c.alpha = c.alpha.to(DEV)
    return c


_BATCH = {}


def _batch(B=4, N=256):
    """One fixed batch (source clouds, labels, target clouds, labels) on the host, made once and never written to."""
    if (B, N) not in _BATCH:
        g = torch.Generator().manual_seed(17)
        _BATCH[(B, N)] = (O.synth_clouds(B, N, g), torch.randint(0, 10, (B,), generator=g),
                          O.synth_clouds(B, N, g), torch.randint(0, 10, (B,), generator=g))
    return [t.to(DEV) for t in _BATCH[(B, N)]]


def _sha(net):
    h = hashlib.sha256()
    for k, v in sorted(net.state_dict().items()):
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ 5. SUGStep
_SUG_CASES = {'class_weighting_target_loss': (_class_weighting, {'TARGET_LOSS': 1.0}),
              'focal_adv': (_focal, {'ADV_WEIGHT': 0.5, 'TARGET_LOSS': 0.0})}


@pytest.mark.parametrize('pair_domains', [True, False])
@pytest.mark.parametrize('case', sorted(_SUG_CASES))
def test_sug_step_with_the_fused_cls_loss_tail_equals_the_composed_step(case, pair_domains, monkeypatch):
    """tests/test_gpu_loss.py::test_step_with_fused_loss_tail_equals_the_unfused_step for the criteria of the shipped
    configurations, on Net_MDA('Pointnet'), 4 clouds per domain, N = 256: SUG_FUSED_LOSS=1 (ops.cls_loss) against =0 (the
    criterion module, discrepancy() and the scalar algebra from torch ops), same losses and gradients."""
    from bench import BENCH_METHODS
    from sug_amd import ops
    from sug_amd.train_step import SUGStep
    make, extra = _SUG_CASES[case]
    methods = dict(BENCH_METHODS, **extra)
    res = []
    for fused in ('1', '0'):
        monkeypatch.setenv('SUG_FUSED_LOSS', fused)
        net = _net()
        tr = SUGStep(net, lr=0.0, weight_decay=0.0, methods=methods, criterion=make(), pair_domains=pair_domains)
        data = _batch()
        torch.manual_seed(5)
        fused_before = tr.fused_heads
        tr.fused_heads = True
        keep, ops.FUSED_HEADS = ops.FUSED_HEADS, True
        try:
            lc, lg, ls = tr.losses(*data, combine=(fused == '1'))
            tot = tr._total if tr._total is not None else lc + lg + ls
            tr._total = None
            tot.backward()
        finally:
            ops.FUSED_HEADS = keep
            tr.fused_heads = fused_before
        assert tr.loss_form == ('cls_loss' if fused == '1' else 'composed')
        res.append(([float(v.detach()) for v in (lc, lg, ls, tot)],
                    {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    print(case, pair_domains, res[0][0], res[1][0])
    for a, b in zip(res[0][0], res[1][0]):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), (res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys()
    gmax = max(float(g.abs().max()) for g in res[1][1].values())
    for k in res[1][1]:
        torch.testing.assert_close(res[0][1][k], res[1][1][k], rtol=2e-4, atol=2e-6 * gmax)


def test_plain_cross_entropy_keeps_the_ce_pair_tail():
    from bench import BENCH_METHODS
    from sug_amd.train_step import SUGStep
    tr = SUGStep(_net(), lr=0.0, weight_decay=0.0, methods=BENCH_METHODS)
    tr.losses(*_batch(), combine=True)
    tr._total = None
    assert tr.loss_form == 'ce_pair'


# ------------------------------------------------------------------------------------------------ 6. graph replay
def _sug_run(use_graph, steps=4, new_alpha_at=None):
    from bench import BENCH_METHODS
    from sug_amd.train_step import SUGStep
    net = _net()
    crit = _class_weighting()
    tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=use_graph, methods=dict(BENCH_METHODS, TARGET_LOSS=1.0), criterion=crit)
    batch = _batch()
    torch.manual_seed(3)
    out = []
    for i in range(steps):
        if i == new_alpha_at:
            crit.alpha = torch.tensor(WEIGHTS[::-1], device=DEV)
        out.append(([float(v) for v in tr.step(*batch)], _sha(net)))
        assert tr.loss_form == 'cls_loss'
    return out, tr


def test_sug_graph_replay_equals_the_eager_twin_bit_for_bit():
    """Four steps (planning step, capture, two replays) with CLS_LOSS ClassWeighting and TARGET_LOSS 1: the losses of every step
    and a hash over all parameters and buffers after it equal those of the eager launches."""
    a, _ = _sug_run(False)
    b, tr = _sug_run(True)
    assert a == b, 'graph replay differs from eager: %s vs %s' % ([x[0] for x in a], [x[0] for x in b])
    assert len(tr._graphs) == 1 and all(np.isfinite(x[0]).all() for x in a)


def test_a_changed_alpha_is_captured_anew_not_replayed_stale():
    """criterion.alpha replaced after the third step: the record in the graph key changes, so the fourth step plans a new key
    (eagerly, uploading the new weights) and the fifth captures it; the trajectory is the eager one's."""
    a, _ = _sug_run(False, steps=6, new_alpha_at=3)
    b, tr = _sug_run(True, steps=6, new_alpha_at=3)
    assert a == b, 'graph replay differs from eager: %s vs %s' % ([x[0] for x in a], [x[0] for x in b])
    assert len(tr._graphs) == 2
    same, _ = _sug_run(False, steps=4)
    assert a[:3] == same[:3] and a[3] != same[3]            # the new weights do change the step


# ------------------------------------------------------------------------------------------------ 7. UDAStep
def _uda_one_step(**kw):
    from sug_amd.uda_step import UDAStep
    net = _net()
    tr = UDAStep(net, recipe='naive_mmd', target_loss=1.0, criterion=_focal(2), lr=0.0, use_graph=False, fused_adam=False, **kw)
    torch.manual_seed(5)
    from sug_amd import ops
    with ops.CTX.scoped(fused_heads=True):                  # (fused_loss=False alone would also unfuse the heads' LayerNorm)
        losses = [float(v) for v in tr.step(*_batch())]
    names = {id(p): k for k, p in net.named_parameters()}
    grads = {}
    for tag, opt in (('g', tr.optimizer_g), ('c', tr.optimizer_c), ('dis', tr.optimizer_dis)):
        for p, st in opt.state.items():
            grads[tag + ':' + names[id(p)]] = st['exp_avg'].detach().clone() * 10.0      # exp_avg = 0.1 * grad after one step
    return losses, grads, tr


def test_uda_step_with_focal_loss_takes_the_fused_tail():
    """UDAStep('naive_mmd', target_loss=1.0) with focal_loss(gamma=2): fused_loss=True (ops.cls_loss) against False (composed),
    learning rate 0 so that phase 2 of both runs on the same weights, the heads' fused LayerNorm + activation in both; the
    gradients are read from Adam's first moments."""
    a = _uda_one_step(fused_loss=False)
    b = _uda_one_step(fused_loss=True)
    assert a[2].loss_form == 'composed' and b[2].loss_form == 'cls_loss'
    print(a[0], b[0])
    for x, y in zip(b[0], a[0]):
        assert abs(x - y) <= 2e-6 * max(1.0, abs(y)), (a[0], b[0])
    assert a[1].keys() == b[1].keys()
    gmax = max(float(g.abs().max()) for g in a[1].values())
    for k in a[1]:
        torch.testing.assert_close(b[1][k], a[1][k], rtol=2e-4, atol=2e-6 * gmax)


def test_uda_books_with_focal_loss_are_the_sums_of_loss_times_rows():
    from sug_amd.uda_step import UDAStep
    net = _net()
    tr = UDAStep(net, recipe='naive_mmd', target_loss=1.0, criterion=_focal(2))
    torch.manual_seed(11)
    want, batch = [0.0, 0.0, 0.0], _batch()
    for rows in (4, 4, 3, 4, 4, 3):                         # two graph keys
        ls = tr.step(*[t[:rows] for t in batch])
        assert tr.loss_form == 'cls_loss'
        for j in range(3):
            want[j] += float(ls[j]) * rows
    assert tr.stats == {'planned': 2, 'captured': 2, 'replayed': 4, 'refused': 0}, (tr.stats, tr.why)      # steps 1 3 4 and 5
    got = tr.epoch_totals()
    assert got[3] == got[4] == 22.0
    for a, b in zip(got[:3], want):
        assert abs(a - b) <= 4 * np.finfo(np.float64).eps * abs(b), (got, want)
