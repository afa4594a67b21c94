"""GPU: the class-aligned MMD with its row selection on the device (ops.class_pairs / ops.class_mmd = sug_mmd_select,
sug_class_mmd_fwd / _bwd; mmd.hard_mmd and mmd.max_hard_mmd(pairing='stable')).

  1. the index kernel against mmd.class_pairs_host, exactly;
  2. values and gradients against the fp64 oracle on the CPU (tolerances of tests/test_gpu_mmd.py), the n == 0 contract, exact
     zeros on unselected rows, and the composed path mix_rbf_mmd2(feat_s[idx_s], feat_t[idx_t]) on the same device: gradients
     bit for bit, values to 1e-6 (the three fp64 sums are accumulated by workgroup in no fixed order);
  3. mmd_cal's routing;
  4. replay: SUGStep / UDAStep steps configured with HARD_MMD or MAX_HARD_MMD + PAIRING: stable are captured, and ONE captured
     step serves batches with different n (n == 0 included) like its eager twin."""
import functools

import pytest
import torch

from class_mmd_cases import label_sets, mixed_labels, random_labels
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = dict(rtol=1e-4, atol=1e-5)                                # tests/test_gpu_mmd.py's


# ------------------------------------------------------------------------------------------------ 1. the index kernel
def _check_pairs(ls, lt, mode, num_class):
    from sug_amd import ops
    from sug_amd.model import mmd
    m = ls.numel()
    want_s, want_t = mmd.class_pairs_host(ls, lt, mode, num_class)
    idx_s, idx_t, n = ops.class_pairs(ls.to(DEV), lt.to(DEV), mode, num_class)
    assert idx_s.dtype == idx_t.dtype == n.dtype == torch.int32 and idx_s.shape == idx_t.shape == (m,) and n.dim() == 0
    assert int(n) == len(want_s)
    assert idx_s.cpu().tolist() == want_s + [-1] * (m - len(want_s))
    assert idx_t.cpu().tolist() == want_t + [-1] * (m - len(want_t))
    _, _, pos_s, pos_t, _ = ops._class_select(ls.to(DEV), lt.to(DEV), mode, num_class)          # the inverse maps
    for pos, want in ((pos_s, want_s), (pos_t, want_t)):
        inv = [-1] * m
        for p, i in enumerate(want):
            inv[i] = p
        assert pos.cpu().tolist() == inv


@pytest.mark.parametrize('num_class', [10, 40])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('name,ls,lt,in_range', label_sets(), ids=[s[0] for s in label_sets()])
def test_class_pairs_equal_the_host_rule(name, ls, lt, in_range, mode, num_class):
    _check_pairs(ls, lt, mode, num_class)


@pytest.mark.parametrize('mode', [0, 1])
def test_class_pairs_at_the_row_limit_and_beyond(mode):
    from sug_amd import ops
    ls, lt = random_labels(1024, hi=40)
    _check_pairs(ls, lt, mode, 40)
    _check_pairs(ls, lt, mode, 10)                               # labels 10 .. 39 are out of range here
    ls[5], lt[5] = 2 ** 40 + 3, 2 ** 40 + 3                      # beyond 32 bits: equal row by row, no class
    _check_pairs(ls, lt, mode, 64)
    z = torch.zeros(1025, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match='m=1025'):
        ops.class_pairs(z, z, mode)
    with pytest.raises(RuntimeError, match='num_class=65'):
        ops.class_pairs(z[:4], z[:4], mode, 65)
    with pytest.raises(RuntimeError, match='mode'):
        ops.class_pairs(z[:4], z[:4], 2)
    X = torch.zeros(1025, 8, device=DEV)
    assert not ops.class_mmd_supported(z, X, z, X) and ops.class_mmd_supported(z[:1024], X[:1024], z[:1024], X[:1024])
    assert not ops.class_mmd_supported(z[:4], X[:4], z[:4], X[:4], num_class=65)
    assert not ops.class_mmd_supported(z[:4], X[:4].double(), z[:4], X[:4].double())
    assert not ops.class_mmd_supported(z[:4], X[:4], z[:4], X[:4], sigmas=tuple(range(1, 10)))


# ------------------------------------------------------------------------------------------------ 2. values and gradients
SHAPES = [(5, 7), (8, 256), (32, 4096), (33, 266), (80, 266)]
KINDS = ['same', 'one', 'disjoint', 'mixed']


@functools.lru_cache(maxsize=None)
def _features(m, D):
    """tests/test_gpu_mmd.py::test_mmd_vs_oracle_sizes' recipe."""
    g = torch.Generator().manual_seed(m + D)
    X = torch.randn(m, D, generator=g) * (0.05 if D > 1000 else 1.0)
    Y = torch.randn(m, D, generator=g) * (0.05 if D > 1000 else 1.0) + 0.02
    return X, Y


@functools.lru_cache(maxsize=None)
def _labels(m, kind):
    """(label_s, label_t, n under the hard rule, n under the stable rule) -- the n as the constructions intend them."""
    g = torch.Generator().manual_seed(50 + m)
    ls = torch.randint(0, 10, (m,), generator=g)
    if kind == 'same':
        return ls, ls.clone(), m, m
    if kind == 'one':                                           # row m // 2 keeps its label, every other target label is 10 + ...
        lt = ls + 10
        lt[m // 2] = ls[m // 2]
        return ls, lt, 1, 1
    if kind == 'disjoint':
        return ls % 5, ls % 5 + 5, 0, 0
    ls, lt = mixed_labels(m)
    return ls, lt, None, None


@functools.lru_cache(maxsize=None)
def _reference(m, D, kind, mode):
    """fp64 on the CPU, once per case: (value, d feat_s, d feat_t, ind_s, ind_t as index tensors).  mode 0: oracle.ref_cpu.mmd_cal(HARD_MMD);
    mode 1: O.mix_rbf_mmd2 on class_pairs_host's rows."""
    from sug_amd.model import mmd
    X, Y = _features(m, D)
    ls, lt, _, _ = _labels(m, kind)
    ind_s, ind_t = (torch.tensor(i, dtype=torch.int64) for i in mmd.class_pairs_host(ls, lt, mode))
    Xo, Yo = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    if mode == 0:
        v = O.mmd_cal(ls, Xo, lt, Yo, {'NAME': 'HARD_MMD'})
    else:
        v = O.mix_rbf_mmd2(Xo[ind_s], Yo[ind_t])
    v.backward()
    return v.detach(), Xo.grad, Yo.grad, ind_s, ind_t


def _check_case(m, D, kind, mode, strided=False):
    from sug_amd import ops
    from sug_amd.model import mmd
    X, Y = _features(m, D)
    ls, lt, n0, n1 = _labels(m, kind)
    vo, gxo, gyo, ind_s, ind_t = _reference(m, D, kind, mode)
    n = int(ind_s.numel())
    if kind == 'mixed':
        assert 0 < n < m, (m, mode, n)
    else:
        assert n == (n0, n1)[mode], (kind, mode, n)
    if strided:                                                 # feature blocks as the left halves of [m, 2D] tensors
        Xw, Yw = torch.zeros(m, 2 * D), torch.zeros(m, 2 * D)
        Xw[:, :D], Yw[:, :D] = X, Y
        Xw, Yw = Xw.to(DEV).requires_grad_(True), Yw.to(DEV).requires_grad_(True)
        Xg, Yg = Xw[:, :D], Yw[:, :D]
        assert Xg.stride(0) == 2 * D
    else:
        Xw, Yw = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
        Xg, Yg = Xw, Yw
    lsg, ltg = ls.to(DEV), lt.to(DEV)
    other = torch.full((3,), 0.5, device=DEV, requires_grad=True)
    v = ops.class_mmd(lsg, Xg, ltg, Yg, mode)
    assert v.dim() == 0 and v.dtype == torch.float32
    ((other * other).sum() + 2.0 * v).backward()
    gx, gy = (Xw.grad[:, :D], Yw.grad[:, :D]) if strided else (Xw.grad, Yw.grad)
    print('m=%d D=%d %s mode %d n=%d: value %r fp64 %r' % (m, D, kind, mode, n, float(v.detach()), float(vo)))
    assert torch.equal(other.grad, torch.ones(3, device=DEV))  # 2 * 0.5, whatever the MMD term is
    sel_s, sel_t = torch.zeros(m, dtype=torch.bool), torch.zeros(m, dtype=torch.bool)
    sel_s[ind_s], sel_t[ind_t] = True, True
    for g_, sel in ((gx, sel_s), (gy, sel_t)):                  # unselected rows: exact zeros, and no NaN anywhere
        assert not bool(torch.isnan(g_).any())
        assert float(g_.cpu()[~sel].abs().sum()) == 0.0
    if strided:
        assert float(Xw.grad[:, D:].abs().sum()) == 0.0 and float(Yw.grad[:, D:].abs().sum()) == 0.0
    if n == 0:
        assert bool(torch.isnan(v)) and bool(torch.isnan(vo))
        assert float(gx.abs().sum()) == 0.0 and float(gy.abs().sum()) == 0.0
        assert float(gxo.abs().sum()) == 0.0 and float(gyo.abs().sum()) == 0.0 and not bool(torch.isnan(gxo).any())
        return
    torch.testing.assert_close(v.detach().cpu().double(), vo, **TOL)
    s = max(float(gxo.abs().max()), float(gyo.abs().max()))
    torch.testing.assert_close(gx.cpu().double() / 2.0, gxo, rtol=1e-3, atol=2e-4 * s)
    torch.testing.assert_close(gy.cpu().double() / 2.0, gyo, rtol=1e-3, atol=2e-4 * s)
    # the composed path on the same device: the same per-pair arithmetic and backward body
    Xc, Yc = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
    vc = mmd.mix_rbf_mmd2(Xc[ind_s.to(DEV)], Yc[ind_t.to(DEV)], mmd.sigma_list)
    (2.0 * vc).backward()
    torch.testing.assert_close(v.detach(), vc.detach(), rtol=1e-6, atol=0.0)
    assert torch.equal(gx, Xc.grad) and torch.equal(gy, Yc.grad), (float((gx - Xc.grad).abs().max()), float((gy - Yc.grad).abs().max()))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('m,D', SHAPES)
def test_class_mmd_values_and_gradients(m, D, kind, mode):
    """(80, 266) with label_t = label_s is the one case with 2n > 128 at D >= 256 (the tiled form where a smaller n takes the
    4 x 4 form); (5, 7) is the tiled form at D < 256; (33, 266) has ragged tiles in both forms."""
    _check_case(m, D, kind, mode)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('kind', ['mixed', 'disjoint'])
def test_class_mmd_feature_blocks_with_a_row_stride(kind, mode):
    _check_case(33, 266, kind, mode, strided=True)


def test_class_mmd_without_a_gradient_and_for_one_side():
    from sug_amd import ops
    m, D = 33, 266
    X, Y = (t.to(DEV) for t in _features(m, D))
    ls, lt = (t.to(DEV) for t in _labels(m, 'mixed')[:2])
    v0 = ops.class_mmd(ls, X, lt, Y, 1)
    assert not v0.requires_grad
    Yr = Y.clone().requires_grad_(True)
    v1 = ops.class_mmd(ls, X, lt, Yr, 1)
    v1.backward()
    both_x, both_y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    ops.class_mmd(ls, both_x, lt, both_y, 1).backward()
    assert torch.equal(Yr.grad, both_y.grad) and float(both_x.grad.abs().max()) > 0.0
    torch.testing.assert_close(v0, v1.detach(), rtol=1e-6, atol=0.0)


# ------------------------------------------------------------------------------------------------ 3. mmd_cal's routing
def test_mmd_cal_routes_the_class_aligned_names(monkeypatch, mmd_golden):
    from sug_amd import ops
    from sug_amd.model import mmd
    calls = []
    real = ops.class_mmd
    monkeypatch.setattr(ops, 'class_mmd', lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1])
    G = mmd_golden
    X, Y = G['sem32_X'].to(DEV), G['sem32_Y'].to(DEV)
    ls, lt = G['sem32_ls'].to(DEV), G['sem32_lt'].to(DEV)
    v = mmd.mmd_cal(ls, X, ls.clone(), Y, {'NAME': 'HARD_MMD'})
    assert calls == [0]
    torch.testing.assert_close(v.cpu(), G['sem32_hard'], **TOL)
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'MAX_HARD_MMD', 'PAIRING': 'stable'})
    assert calls == [0, 1]
    ind_s, ind_t = mmd.class_pairs_host(G['sem32_ls'], G['sem32_lt'], 1)
    want = O.mix_rbf_mmd2(G['sem32_X'].double()[ind_s], G['sem32_Y'].double()[ind_t])
    torch.testing.assert_close(v.cpu().double(), want, **TOL)
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'MAX_HARD_MMD'})
    assert calls == [0, 1]                                      # the default pairing stays the host path
    torch.testing.assert_close(v.cpu(), G['sem32_maxhard'], **TOL)
    torch.testing.assert_close(mmd.max_hard_mmd(ls, X, lt, Y).cpu(), G['sem32_maxhard'], **TOL)
    assert calls == [0, 1]
    with pytest.raises(RuntimeError, match='pairing'):
        mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'MAX_HARD_MMD', 'PAIRING': 'nope'})


def test_knob_off_restores_the_composed_lines(monkeypatch):
    """SUG_CLASS_MMD=0 (ops.CLASS_MMD, read at import): hard_mmd is boolean indexing + mix_rbf_mmd2 again -- the same value and,
    bit for bit, the same gradients -- and pairing='stable' says that it needs the device path."""
    from sug_amd import ops
    from sug_amd.model import mmd
    m, D = 33, 266
    ls, lt = (t.to(DEV) for t in _labels(m, 'mixed')[:2])
    res = []
    for on in (True, False):
        monkeypatch.setattr(ops, 'CLASS_MMD', on)
        calls = []
        real = ops.class_mmd
        monkeypatch.setattr(ops, 'class_mmd', lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1])
        X, Y = (t.to(DEV).requires_grad_(True) for t in _features(m, D))
        v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'HARD_MMD'})
        v.backward()
        assert calls == ([0] if on else [])
        res.append((v.detach(), X.grad, Y.grad))
        monkeypatch.setattr(ops, 'class_mmd', real)
    torch.testing.assert_close(res[0][0], res[1][0], rtol=1e-6, atol=0.0)
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    with pytest.raises(RuntimeError, match='stable'):
        mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'MAX_HARD_MMD', 'PAIRING': 'stable'})


# ------------------------------------------------------------------------------------------------ 4. replay
def _net(name='DGCNN', wseed=5):
    from sug_amd.model.Model import Net_MDA
    net = Net_MDA(name)
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, wseed))
    for mod in net.modules():
        if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)):
            mod.p = 0.0
    return net.to(DEV).train()


_LS = [0, 1, 2, 3]
_LT = {3: [0, 1, 2, 9], 0: [9, 8, 7, 6], 4: [0, 1, 2, 3], 2: [0, 9, 8, 3]}     # hard n -> target labels against _LS


@functools.lru_cache(maxsize=None)
def _clouds(B=4, N=1024):
    g = torch.Generator().manual_seed(11)
    return [(O.synth_clouds(B, N, g), O.synth_clouds(B, N, g)) for _ in range(4)]


def _batches(ns, mode):
    from sug_amd.model import mmd
    out = []
    for (data, data_t), n in zip(_clouds(), ns):
        ls, lt = torch.tensor(_LS), torch.tensor(_LT[n])
        assert len(mmd.class_pairs_host(ls, lt, mode)[0]) == n
        out.append([t.to(DEV) for t in (data, ls, data_t, lt)])
    return out


def _sug_run(cfg, ns, mode, use_graph):
    from sug_amd.train_step import SUGStep
    net = _net()
    methods = {'GEO_MMD': [dict(cfg, GEO_SCALE=1)], 'SEM_MMD': [dict(cfg, SEM_SCALE=1)]}
    tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=use_graph, methods=methods)
    torch.manual_seed(3)
    losses = torch.stack([torch.stack([v.clone() for v in tr.step(*b)]) for b in _batches(ns, mode)]).cpu()
    return tr, net, losses


def _same_as_twin(e_net, g_net, e_loss, g_loss, ns):
    for (k, a), (_, b) in zip(e_net.state_dict().items(), g_net.state_dict().items()):
        assert torch.equal(a, b), k
    assert all(bool(torch.isfinite(p).all()) for p in g_net.parameters())
    nan_rows = torch.tensor([n == 0 for n in ns])
    for loss in (e_loss, g_loss):                               # the MMD columns: NaN exactly at the n == 0 steps
        assert torch.equal(torch.isnan(loss[:, 1:]).all(dim=1), nan_rows) and torch.equal(torch.isnan(loss[:, 1:]).any(dim=1), nan_rows)
        assert bool(torch.isfinite(loss[:, 0]).all())
    ok = ~nan_rows
    torch.testing.assert_close(g_loss[ok], e_loss[ok], rtol=1e-6, atol=0.0)


@pytest.mark.parametrize('cfg,ns,mode', [({'NAME': 'HARD_MMD'}, (3, 0, 4, 2), 0),
                                          ({'NAME': 'MAX_HARD_MMD', 'PAIRING': 'stable'}, (3, 0), 1)],
                         ids=['hard', 'max_hard_stable'])
def test_sug_step_is_captured_and_one_graph_serves_every_n(cfg, ns, mode):
    """SUGStep(use_graph=True) with both MMD entries class-aligned: planned on the first step, captured on the second (the
    n == 0 batch), replayed for the others -- one graph -- and equal to the eager twin: parameters bit for bit, the reported
    MMD values to 1e-6, NaN exactly where no row matches.  (Before ops.class_mmd the capture failed on nonzero's host wait.)
    SUGStep keeps its captured steps in `_graphs` and has no `stats` / `why` of ReplayedStep's kind (a failed capture raises
    there): one key with a captured graph is its statement of planned 1, captured 1, refused 0."""
    e_tr, e_net, e_loss = _sug_run(cfg, ns, mode, False)
    g_tr, g_net, g_loss = _sug_run(cfg, ns, mode, True)
    assert len(g_tr._graphs) == 1
    st = next(iter(g_tr._graphs.values()))
    assert st['graph'] is not None
    if hasattr(g_tr, 'stats'):
        assert g_tr.stats['planned'] == 1 and g_tr.stats['captured'] == 1 and g_tr.stats['refused'] == 0 and g_tr.why is None
    _same_as_twin(e_net, g_net, e_loss, g_loss, ns)


def test_uda_step_with_a_hard_class_mmd_is_captured():
    from sug_amd.uda_step import UDAStep
    ns, res = (3, 0), {}
    for use_graph in (False, True):
        net = _net()
        tr = UDAStep(net, 'naive_mmd', class_mmd={'NAME': 'HARD_MMD'}, lr=1e-3, weight_decay=5e-5, use_graph=use_graph)
        torch.manual_seed(3)
        losses = torch.stack([torch.stack(tr.step(*b)) for b in _batches(ns, 0)]).cpu()
        res[use_graph] = (tr, net, losses)
    tr = res[True][0]
    assert tr.stats == {'planned': 1, 'captured': 1, 'replayed': 1, 'refused': 0} and tr.why is None, (tr.stats, tr.why)
    e_loss, g_loss = res[False][2], res[True][2]
    for (k, a), (_, b) in zip(res[False][1].state_dict().items(), res[True][1].state_dict().items()):
        assert torch.equal(a, b), k
    assert all(bool(torch.isfinite(p).all()) for p in res[True][1].parameters())
    for loss in (e_loss, g_loss):                               # loss_node: finite at n = 3, NaN at n = 0
        assert bool(torch.isfinite(loss[0]).all()) and bool(torch.isnan(loss[1, 2])) and bool(torch.isfinite(loss[1, :2]).all())
    torch.testing.assert_close(g_loss[0], e_loss[0], rtol=1e-6, atol=0.0)
    torch.testing.assert_close(g_loss[1, :2], e_loss[1, :2], rtol=1e-6, atol=0.0)
