"""GPU: the contrastive alignment mode NAME: CL on HIP (ops.cl_loss / ops.cl_loss_multi = sug_cl_loss_fwd / _bwd;
mmd.contrastive_loss_weighted, mmd_cal, mmd.cl_loss_multi, SUGStep).

  1. values and 2. gradients of every case of tests/golden/cl_loss.npz against the reference's fp64 results, within twice the
     reference's own fp32 error or 1e-4 / 2e-4 of the scale (the bound form of tests/test_gpu_mmd_estimators.py);
  3. a row stride, 4. a row alone and in its batch, 5. several terms in one launch set, 6. one-sided / no gradients,
  7. repeat and graph replay: bit for bit;
  8. routing through the mirror and the SUG_CL_LOSS knob;
  9. SUGStep with NAME: CL entries: planned, captured, replayed, equal to its eager twin bit for bit; a mixed configuration.

Every test prints its figures before it asserts them.  Measured on an MI355X (DESIGN 5f has the table): over the 189 fixture
cases the worst value error is 4.7e-8 (3.2e-4 of its bound) and the worst gradient error 2.6e-4 of its bound -- the one fp32
rounding of the outputs; the zero-row case has a gradient error of 1.4e-2 at a scale of 3.4e5 (bound 67.5)."""
import functools

import pytest
import torch

import cl_loss_cases as C
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _run(ls, X, lt, Y, margin, w, upstream=1.0):
    """(value, d X, d Y) of ops.cl_loss on the device."""
    from sug_amd import ops
    ls, X, lt, Y, w = _dev(ls, X, lt, Y, w)
    X.requires_grad_(True), Y.requires_grad_(True)
    v = ops.cl_loss(ls, X, lt, Y, margin, w)
    assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
    (upstream * v).backward()
    return v.detach(), X.grad, Y.grad


def _check(tag, got, ref64, rec):
    """Bounds 1 and 2 for one case; prints every figure before asserting it.  Returns (value error, its bound, gradient error,
    its bound)."""
    v, gx, gy = got
    v64, g64 = ref64
    _, rec64, val_err, grad_err, grad_scale = rec
    assert abs(float(v64) - rec64) <= 1e-12 * max(1.0, abs(rec64))             # the recomputed fp64 reference is the recorded one
    ev, bv = abs(float(v) - float(v64)), max(2 * val_err, 1e-4 * max(1.0, abs(float(v64))))
    eg = float((torch.cat((gx, gy), 0).cpu().double() - g64).abs().max())
    bg = max(2 * grad_err, 2e-4 * grad_scale)
    print('%s: value %.9g fp64 %.9g err %.3g bound %.3g | gradient err %.3g bound %.3g (scale %.3g)'
          % (tag, float(v), float(v64), ev, bv, eg, bg, grad_scale))
    assert ev <= bv, (tag, ev, bv)
    assert eg <= bg, (tag, eg, bg)
    return ev, bv, eg, bg


# ------------------------------------------------------------------------------------------ 1, 2. values and gradients
@pytest.mark.parametrize('si', range(len(C.shapes())), ids=C.shape_ids())
def test_values_and_gradients_against_the_fp64_reference(si):
    worst = [0.0, 0.0]
    for vi, (li, margin, wi) in enumerate(C.variants()):
        r = _check('%s labels %d margin %g weights %d' % (C.shape_ids()[si], li, margin, wi), _run(*C.case(si, vi)), C.ref64(si, vi),
                   C.recorded(si, vi))
        worst = [max(worst[0], r[0] / r[1]), max(worst[1], r[2] / r[3] if r[3] > 0 else 0.0)]
    print('%s: worst value err / bound %.3g, worst gradient err / bound %.3g' % (C.shape_ids()[si], worst[0], worst[1]))


@pytest.mark.parametrize('name', C.DEGENERATE)
def test_degenerate_rows(name):
    """A zero source row (cos = 0, a finite gradient of order 1e6 times the other row's) and x_i == y_i on positive pairs (a
    loss of order 1e-13): the bounds of the other cases, and every gradient entry finite."""
    got = _run(*C.degenerate(name))
    assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[2]).all())
    _check(name, got, C.degenerate_ref64(name), C.degenerate_recorded(name))
    if name == 'zero':
        assert float(got[1][0].abs().max()) > 1e5 * float(got[1][1].abs().max()) and float(got[2][0].abs().max()) == 0.0
    else:
        assert 0.0 <= float(got[0]) < 1e-11


def test_more_rows_than_the_fold_has_threads():
    """m = 300: the fold's 256 threads take a second row each (no fixture case is that tall); reference: the composed lines
    in fp64 on the CPU; bound: 1e-4 / 2e-4 of the scale, the form of bounds 1 and 2 without the reference's fp32 error."""
    g = torch.Generator().manual_seed(300)
    m, D = 300, 5
    X = torch.randn(m, D, generator=g)
    Y = 0.5 * X + torch.randn(m, D, generator=g)
    ls = torch.randint(0, 10, (m,), generator=g)
    lt = torch.where(torch.arange(m) % 3 == 0, ls, (ls + 1) % 10)
    w = torch.rand(1, m, generator=g) + 0.5
    cos = torch.nn.functional.cosine_similarity(X.double(), Y.double())
    assert float((cos - 0.2).abs().min()) >= 1e-4
    v64, g64 = C.composed(ls, X, lt, Y, 0.2, w)
    v, gx, gy = _run(ls, X, lt, Y, 0.2, w)
    ev, eg, scale = abs(float(v) - float(v64)), float((torch.cat((gx, gy), 0).cpu().double() - g64).abs().max()), float(g64.abs().max())
    print('m=300: value %.9g fp64 %.9g err %.3g | gradient err %.3g scale %.3g' % (float(v), float(v64), ev, eg, scale))
    assert ev <= 1e-4 * max(1.0, abs(float(v64))) and eg <= 2e-4 * scale
    from sug_amd import ops
    one = ops.cl_loss_cos(X[299:300].to(DEV), Y[299:300].to(DEV))
    assert torch.equal(ops.cl_loss_cos(X.to(DEV), Y.to(DEV))[299:300], one)


# ------------------------------------------------------------------------------------------------------ 3. row stride
@pytest.mark.parametrize('D', [70, 256, 257])
@pytest.mark.parametrize('off', [0, 1])
def test_row_stride_gives_the_bits_of_the_contiguous_copy(D, off):
    """Features as column slices of a wider buffer, ld = D + 3 (rows off the 16-byte grid; with off = 1 the base as well),
    against their contiguous copies -- at D = 256 those take the 16-byte loads, the views the 4-byte ones."""
    from sug_amd import ops
    si = C.shapes().index((33, 257))
    ls, X, lt, Y, margin, w = C.case(si, 4)
    X, Y = X[:, :D].contiguous(), Y[:, :D].contiguous()
    want = _run(ls, X, lt, Y, margin, w, upstream=0.5)
    m = X.shape[0]
    bx, by = torch.zeros(m, D + 3), torch.zeros(m, D + 3)
    bx[:, off:off + D], by[:, off:off + D] = X, Y
    bx, by = bx.to(DEV).requires_grad_(True), by.to(DEV).requires_grad_(True)
    vx, vy = bx[:, off:off + D], by[:, off:off + D]
    assert vx.stride(0) == D + 3 and not vx.is_contiguous()
    lsd, ltd, wd = _dev(ls, lt, w)
    v = ops.cl_loss(lsd, vx, ltd, vy, margin, wd)
    (0.5 * v).backward()
    assert torch.equal(v.detach(), want[0])
    for buf, g in ((bx, want[1]), (by, want[2])):
        assert torch.equal(buf.grad[:, off:off + D], g)
        outside = torch.ones(D + 3, dtype=torch.bool)
        outside[off:off + D] = False
        assert float(buf.grad[:, outside.to(DEV)].abs().sum()) == 0.0
    assert float(want[1].abs().max()) > 0.0 and float(want[2].abs().max()) > 0.0


# ----------------------------------------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize('m,D', [(65, 70), (3, 4099)])
def test_a_row_has_the_same_cos_alone_and_in_its_batch(m, D):
    """The saved per-row cos (fp64, the fold's field) of every row taken alone, m = 1, has the bits it has in the batch."""
    from sug_amd import ops
    _, X, _, Y, _, _ = C.case(C.shapes().index((m, D)), 0)
    X, Y = _dev(X, Y)
    batch = ops.cl_loss_cos(X, Y)
    assert batch.dtype == torch.float64 and batch.shape == (m,)
    alone = torch.cat([ops.cl_loss_cos(X[i:i + 1], Y[i:i + 1]) for i in range(m)])
    assert torch.equal(batch, alone)
    want = torch.nn.functional.cosine_similarity(X.cpu().double(), Y.cpu().double())
    print('m=%d D=%d: worst |cos - fp64 cos| %.3g' % (m, D, float((batch.cpu() - want).abs().max())))
    assert float((batch.cpu() - want).abs().max()) <= 1e-12


# --------------------------------------------------------------------------------------------------------- 5. multi-term
def _three_terms():
    """Three terms of one batch of 3 rows: D = 4099, 257, 70, margins 0.2, 0.0, 0.5, the last one weighted."""
    ids = [C.shapes().index((3, D)) for D in (4099, 257, 70)]
    ls, _, lt, _, _, _ = C.case(ids[0], 8)                                  # 'mixed' labels
    feats = [C.case(si, 0)[1:4:2] for si in ids]
    w = C.case(ids[2], 2)[5]
    assert w is not None and int((ls == lt).sum()) not in (0, 3)
    return ls, lt, [(feats[0][0], feats[0][1], 0.2, None), (feats[1][0], feats[1][1], 0.0, None), (feats[2][0], feats[2][1], 0.5, w)]


def test_multi_term_has_the_bits_of_the_single_term_calls():
    from sug_amd import ops
    ls, lt, terms = _three_terms()
    ups = (1.0, 0.5, 2.0)
    single = [_run(ls, X, lt, Y, mg, w, upstream=u) for (X, Y, mg, w), u in zip(terms, ups)]
    lsd, ltd = _dev(ls, lt)
    dterms = []
    for X, Y, mg, w in terms + terms[:2]:                                       # five terms: a full launch set and a second one
        Xd, Yd, wd = _dev(X, Y, w)
        dterms.append((Xd.requires_grad_(True), Yd.requires_grad_(True), mg, wd))
    vals = ops.cl_loss_multi(lsd, ltd, dterms)
    assert len(vals) == 5
    sum(u * v for u, v in zip(ups + ups[:2], vals)).backward()
    for i, (v, (Xd, Yd, _, _)) in enumerate(zip(vals, dterms)):
        want = single[i % 3]
        assert torch.equal(v.detach(), want[0]), i
        assert torch.equal(Xd.grad, want[1]) and torch.equal(Yd.grad, want[2]), i
        assert float(Xd.grad.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------ 6. one-sided and no gradient
def test_one_sided_and_no_gradient():
    from sug_amd import ops
    ls, X, lt, Y, margin, w = C.case(C.shapes().index((33, 70)), 4)
    want = _run(ls, X, lt, Y, margin, w)
    lsd, Xd, ltd, Yd, wd = _dev(ls, X, lt, Y, w)
    Xr = Xd.clone().requires_grad_(True)
    v = ops.cl_loss(lsd, Xr, ltd, Yd, margin, wd)
    v.backward()
    assert torch.equal(v.detach(), want[0]) and torch.equal(Xr.grad, want[1])
    Yr = Yd.clone().requires_grad_(True)
    v = ops.cl_loss(lsd, Xd, ltd, Yr, margin, wd)
    v.backward()
    assert torch.equal(v.detach(), want[0]) and torch.equal(Yr.grad, want[2])
    v = ops.cl_loss(lsd, Xd, ltd, Yd, margin, wd)
    assert not v.requires_grad and torch.equal(v, want[0])
    with torch.no_grad():
        v = ops.cl_loss(lsd, Xr, ltd, Yr, margin, wd)
    assert not v.requires_grad and torch.equal(v, want[0])
    # in a launch set, a term without a gradient beside one with (autograd marks every output of the set as differentiable;
    # the first term saves no coefficients and the backward skips it)
    vals = ops.cl_loss_multi(lsd, ltd, [(Xd, Yd, margin, wd), (Xr, Yd, margin, wd)])
    Xr.grad = None
    assert torch.equal(vals[0].detach(), want[0]) and torch.equal(vals[1].detach(), want[0])
    (vals[0] + vals[1]).backward()
    assert torch.equal(Xr.grad, want[1])


# ------------------------------------------------------------------------------------------------ 7. repeat and replay
def test_repeat_and_graph_replay_are_bit_identical():
    from sug_amd import ops
    ls, lt, terms = _three_terms()
    lsd, ltd = _dev(ls, lt)
    data = [[_dev(X * s, Y * s + o, w) for X, Y, _, w in terms] for s, o in ((1.0, 0.0), (0.7, 0.05))]
    margins = [t[2] for t in terms]

    def run(feats):
        leaves = [(X, Y) for X, Y, _ in feats]
        vals = ops.cl_loss_multi(lsd, ltd, [(X, Y, mg, w) for (X, Y, w), mg in zip(feats, margins)])
        grads = torch.autograd.grad(vals[0] + 0.5 * vals[1] + 2.0 * vals[2], [t for pair in leaves for t in pair])
        return [torch.stack(vals).detach()] + list(grads)

    fresh = lambda d: [(X.clone().requires_grad_(True), Y.clone().requires_grad_(True), w) for X, Y, w in d]
    want = [run(fresh(d)) for d in data]
    again = run(fresh(data[0]))
    assert all(torch.equal(a, b) for a, b in zip(want[0], again))
    static = fresh([(X * 0.3 + 0.2, Y * 0.3 - 0.1, w) for X, Y, w in data[0]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # (torch's recipe: one warm-up on a side stream before a capture)
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard(), torch.cuda.graph(graph):
        got = run(static)
    for d, w_ in zip(data, want):
        with torch.no_grad():
            for (Xs, Ys, _), (X, Y, _) in zip(static, d):
                Xs.copy_(X)
                Ys.copy_(Y)
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(got, w_))
    assert not torch.equal(want[0][0], want[1][0])


# ------------------------------------------------------------------------------------------------------------ 8. routing
def test_mirror_routes_to_the_fused_path_and_the_knob_restores_the_composed_lines(monkeypatch):
    from sug_amd import ops
    from sug_amd.model import mmd
    si, vi = C.shapes().index((33, 257)), 4
    ls, X, lt, Y, margin, w = C.case(si, vi)
    want = _run(ls, X, lt, Y, margin, w)
    lsd, ltd, wd = _dev(ls, lt, w)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, 'CL_LOSS', on)
        calls = []
        real = ops.cl_loss
        monkeypatch.setattr(ops, 'cl_loss', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        Xd, Yd = (t.to(DEV).requires_grad_(True) for t in (X, Y))
        v = mmd.contrastive_loss_weighted(lsd, Xd, ltd, Yd, 0.3, C.criterion(margin), sample_weights=wd)
        v.backward()
        v2 = mmd.mmd_cal(lsd, Xd.detach(), ltd, Yd.detach(), {'NAME': 'CL', 'MARGIN': margin}, sample_weights=wd)
        v3 = mmd.mmd_cal(lsd, Xd.detach(), ltd, Yd.detach(), {'NAME': 'CL', 'MARGIN': 0.9}, sample_weights=wd, CL_criterion=C.criterion(margin))
        # a criterion of another kind (a subclass counts as one) takes the composed lines whatever the knob says
        v4 = mmd.contrastive_loss_weighted(lsd, Xd.detach(), ltd, Yd.detach(), 0.3, lambda a, b, t: C.criterion(margin)(a, b, t), wd)
        assert len(calls) == (3 if on else 0)
        res[on] = (v.detach(), Xd.grad, Yd.grad, v2, v3, v4)
        monkeypatch.setattr(ops, 'cl_loss', real)
    fused, composed = res[True], res[False]
    assert all(torch.equal(fused[k], want[k]) for k in range(3))
    assert torch.equal(fused[3], want[0]) and torch.equal(fused[4], want[0])
    _, v64, val_err, grad_err, grad_scale = C.recorded(si, vi)
    bound = max(2 * val_err, 1e-4 * max(1.0, abs(v64)))
    for k, name in ((0, 'composed'), (3, 'composed via mmd_cal'), (5, 'lambda criterion')):
        err = abs(float(composed[k]) - float(fused[0]))
        print('%s: %.9g fused %.9g |difference| %.3g bound %.3g' % (name, float(composed[k]), float(fused[0]), err, bound))
        assert err <= bound
    assert abs(float(fused[5]) - float(fused[0])) <= bound
    g64 = C.ref64(si, vi)[1]
    eg = float((torch.cat(composed[1:3], 0).cpu().double() - g64).abs().max())
    print('composed gradient err %.3g bound %.3g' % (eg, max(2 * grad_err, 2e-4 * grad_scale)))
    assert eg <= max(2 * grad_err, 2e-4 * grad_scale)


def test_mirror_multi_forms_the_weights_of_mmd_cal():
    """mmd.cl_loss_multi: each term's value has the bits of its own mmd_cal call (SEM_WEIGHTS from the head logits, a term
    without weights beside them)."""
    from sug_amd.model import mmd
    ls, lt, terms = _three_terms()
    lsd, ltd = _dev(ls, lt)
    g = torch.Generator().manual_seed(8)
    preds = [_dev(torch.randn(3, 10, generator=g), torch.randn(3, 10, generator=g)) for _ in range(2)]
    sem = {'NAME': 'CL', 'MARGIN': 0.0, 'SEM_WEIGHTS': 'mean2one', 'LABEL_WEIGHT': 0.5}
    tl = [(_dev(terms[0][0])[0], _dev(terms[0][1])[0], {'NAME': 'CL'}, None, None),
          (_dev(terms[1][0])[0], _dev(terms[1][1])[0], sem, preds[0][0], preds[0][1]),
          (_dev(terms[2][0])[0], _dev(terms[2][1])[0], sem, preds[1][0], preds[1][1])]
    vals = mmd.cl_loss_multi(lsd, ltd, tl)
    for v, (fs, ft, args, ds, dt) in zip(vals, tl):
        assert torch.equal(v, mmd.mmd_cal(lsd, fs, ltd, ft, args, data_s=ds, data_t=dt))
    assert not torch.equal(vals[1], mmd.mmd_cal(lsd, tl[1][0], ltd, tl[1][1], {'NAME': 'CL', 'MARGIN': 0.0}))     # the weights count


# --------------------------------------------------------------------------------------------------------------- 9. step
def _net(wseed=5):
    from sug_amd.model.Model import Net_MDA
    net = Net_MDA('DGCNN')
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, wseed))
    for mod in net.modules():
        if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)):
            mod.p = 0.0
    return net.to(DEV).train()


_LS = [0, 1, 2, 3]
# three, two and two positive pairs.  (Negative pairs below the margin contribute 0, and with fewer than two equal labels in
# four the mean SDA distance of the heads exceeds 1, so 'mean2one' truncates its scale -- and every weight -- to 0, as in the
# reference: such batches have the value 0 exactly and would compare nothing.)
_LTS = ([0, 1, 2, 9], [9, 1, 2, 6], [0, 9, 8, 3])
CL_GEO = {'NAME': 'CL', 'GEO_SCALE': 1, 'GEO_WEIGHTS': 'mean2one'}
CL_SEM = {'NAME': 'CL', 'SEM_SCALE': 1, 'SEM_WEIGHTS': 'mean2one', 'LABEL_WEIGHT': 0.5}
SOFT_SEM = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 5, 'SEM_WEIGHTS': 'mean2one', 'LABEL_WEIGHT': 0.5, 'SEM_SCALE': 1}


@functools.lru_cache(maxsize=None)
def _clouds(B=4, N=1024):
    g = torch.Generator().manual_seed(11)
    return [(O.synth_clouds(B, N, g), O.synth_clouds(B, N, g)) for _ in range(3)]


def _batches():
    return [[t.to(DEV) for t in (data, torch.tensor(_LS), data_t, torch.tensor(lt))] for (data, data_t), lt in zip(_clouds(), _LTS)]


def _sug_run(use_graph, spy=None):
    from sug_amd.train_step import SUGStep
    net = _net()
    tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=use_graph, methods={'GEO_MMD': [dict(CL_GEO)], 'SEM_MMD': [dict(CL_SEM)]})
    torch.manual_seed(3)
    losses = torch.stack([torch.stack([v.clone() for v in tr.step(*b)]) for b in _batches()]).cpu()
    return tr, net, losses


def test_sug_step_with_cl_is_captured_and_replays_like_its_eager_twin(monkeypatch):
    """SUGStep(use_graph=True) with GEO_MMD and SEM_MMD both NAME: CL (SDA weights mean2one): planned on the first step,
    captured on the second, replayed on the third -- one graph -- and three steps equal three eager ones from the same initial
    state and draws: losses and every parameter bit for bit.  The three terms go through mmd.cl_loss_multi.  (SUGStep keeps
    its captured steps in `_graphs` and has no `stats` of ReplayedStep's kind: one key with a captured graph is its statement
    of planned 1, captured 1, refused 0.)"""
    from sug_amd.model import mmd
    calls = []
    real = mmd.cl_loss_multi
    monkeypatch.setattr(mmd, 'cl_loss_multi', lambda ls, lt, terms: (calls.append(len(list(terms))), real(ls, lt, terms))[1])
    e_tr, e_net, e_loss = _sug_run(False)
    assert calls == [3, 3, 3]
    g_tr, g_net, g_loss = _sug_run(True)
    assert len(g_tr._graphs) == 1
    st = next(iter(g_tr._graphs.values()))
    assert st['graph'] is not None
    if hasattr(g_tr, 'stats'):
        assert g_tr.stats['planned'] == 1 and g_tr.stats['captured'] == 1 and g_tr.stats['refused'] == 0 and g_tr.why is None
    print('losses (cls, geo, sem) per step, replayed:\n%s\neager:\n%s' % (g_loss, e_loss))
    assert torch.equal(g_loss, e_loss)
    for (k, a), (_, b) in zip(e_net.state_dict().items(), g_net.state_dict().items()):
        assert torch.equal(a, b), k
    assert all(bool(torch.isfinite(p).all()) for p in g_net.parameters())
    assert bool(torch.isfinite(g_loss).all()) and bool((g_loss[:, 1:] != 0).all())


def test_mixed_configuration_goes_term_by_term_through_mmd_cal(monkeypatch):
    """geo CL with semantic SOFT_MMD, one eager step: three mmd_cal calls (no multi-term form takes a mixed set), the CL one
    on the fused single-term path, and the step's reported parts are the sums of what mmd_cal gives for those arguments."""
    from sug_amd import ops
    from sug_amd.model import mmd
    from sug_amd.train_step import SUGStep
    rec, fused = [], []
    real_cal, real_cl = mmd.mmd_cal, ops.cl_loss
    monkeypatch.setattr(mmd, 'mmd_cal', lambda *a, **k: (rec.append((a, k)), real_cal(*a, **k))[1])
    monkeypatch.setattr(ops, 'cl_loss', lambda *a, **k: (fused.append(1), real_cl(*a, **k))[1])
    monkeypatch.setattr(mmd, 'cl_loss_multi', lambda *a, **k: pytest.fail('a mixed set has no multi-term form'))
    monkeypatch.setattr(mmd, 'soft_mmd_multi', lambda *a, **k: pytest.fail('a mixed set has no multi-term form'))
    tr = SUGStep(_net(), lr=1e-3, weight_decay=5e-5, use_graph=False, methods={'GEO_MMD': [dict(CL_GEO)], 'SEM_MMD': [dict(SOFT_SEM)]})
    torch.manual_seed(3)
    out = [v.detach().clone() for v in tr.step(*_batches()[0])]
    assert [a[4]['NAME'] for a, _ in rec] == ['CL', 'SOFT_MMD', 'SOFT_MMD'] and fused == [1]
    monkeypatch.setattr(mmd, 'mmd_cal', real_cal)
    parts = [real_cal(*[t.detach() if isinstance(t, torch.Tensor) else t for t in a],
                      **{k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}) for a, kw in rec]
    M = tr.methods
    want_geo = M['MMD_WEIGHT'] * CL_GEO['GEO_SCALE'] * parts[0]
    want_sem = 0.5 * M['MMD_WEIGHT'] * SOFT_SEM['SEM_SCALE'] * (parts[1] + parts[2])
    print('mixed: geo %.9g from mmd_cal %.9g | sem %.9g from mmd_cal %.9g' % (float(out[1]), float(want_geo), float(out[2]), float(want_sem)))
    torch.testing.assert_close(out[1], want_geo, rtol=1e-6, atol=0.0)
    torch.testing.assert_close(out[2], want_sem, rtol=1e-6, atol=0.0)
    assert bool(torch.isfinite(torch.stack(out)).all()) and float(out[1]) != 0.0 and float(out[2]) != 0.0
