"""CPU: the contrastive alignment mode (NAME: CL) of sug_amd.model.mmd -- the composed lines of contrastive_loss_weighted
against the reference's values recorded in tests/golden/cl_loss.npz, mmd_cal's dispatch (MARGIN, CL_criterion, the weight
precedence, the unknown name), the header / ctypes / Python limits and the host-side checks of sug_cl_loss_fwd / _bwd, and
ops.cl_loss_supported on what it must refuse."""
import ctypes
import inspect
import re

import pytest
import torch
import torch.nn as nn

import cl_loss_cases as C


def test_mirror_has_the_reference_name_and_signature():
    from sug_amd.model import mmd
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(mmd.contrastive_loss_weighted) == [('label_s', E), ('feat_s', E), ('label_t', E), ('feat_t', E), ('label_weight', E),
                                                  ('CL_criterion', E), ('sample_weights', None)]
    assert sig(mmd.mmd_cal)[-1] == ('CL_criterion', None)


@pytest.mark.parametrize('si', range(len(C.shapes())), ids=C.shape_ids())
def test_composed_lines_reproduce_the_recorded_reference(si):
    """fp32 to 1e-6 relative, fp64 to 1e-12 relative, every variant: with and without weights."""
    for vi, (li, margin, wi) in enumerate(C.variants()):
        v32, v64 = C.recorded(si, vi)[:2]
        got32, _ = C.composed(*C.case(si, vi), dtype=torch.float32)
        got64, _ = C.ref64(si, vi)
        assert got32.dtype == torch.float32 and got64.dtype == torch.float64
        assert abs(float(got32) - v32) <= 1e-6 * max(1.0, abs(v32)), (si, vi, float(got32), v32)
        assert abs(float(got64) - v64) <= 1e-12 * max(1.0, abs(v64)), (si, vi, float(got64), v64)
    assert {wi for _, _, wi in C.variants()} == {0, 1, 2}


@pytest.mark.parametrize('name', C.DEGENERATE)
def test_degenerate_cases_as_the_reference_has_them(name):
    v32, v64, _, _, gscale = C.degenerate_recorded(name)
    got64, g64 = C.degenerate_ref64(name)
    got32, _ = C.composed(*C.degenerate(name), dtype=torch.float32)
    assert abs(float(got64) - v64) <= 1e-12 * max(1.0, abs(v64)) and abs(float(got32) - v32) <= 1e-6
    assert bool(torch.isfinite(g64).all())
    assert abs(float(g64.abs().max()) - gscale) <= 1e-11 * gscale
    if name == 'zero':
        assert gscale > 1e5
    else:
        assert 0.0 < v64 < 1e-11


def test_fixture_keeps_every_negative_pair_clear_of_the_margin():
    """The generator's condition, checked again on the stored inputs: |cos - margin| >= 1e-3 on every negative pair."""
    n_active = n_clamped = 0
    for si in range(len(C.shapes())):
        for vi in range(len(C.variants())):
            ls, X, lt, Y, margin, _ = C.case(si, vi)
            X, Y = X.double(), Y.double()
            cos = (X * Y).sum(1) / torch.sqrt(((X * X).sum(1) + 1e-12) * ((Y * Y).sum(1) + 1e-12))
            neg = ls != lt
            assert bool(((cos - margin).abs()[neg] >= 1e-3).all()), (si, vi)
            n_active += int((cos[neg] > margin).sum())
            n_clamped += int((cos[neg] < margin).sum())
    assert n_active > 50 and n_clamped > 50


def _features(m=6, D=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    X, Y = torch.randn(m, D, generator=g), torch.randn(m, D, generator=g)
    ls = torch.arange(m) % 10
    lt = torch.where(torch.arange(m) % 2 == 0, ls, (ls + 1) % 10)
    return ls, X, lt, Y


def _by_hand(ls, X, lt, Y, margin, w=None):
    cos = torch.nn.functional.cosine_similarity(X.double(), Y.double(), dim=1, eps=0.0)
    l = torch.where(ls == lt, 1 - cos, (cos - margin).clamp_min(0))
    if w is not None:
        l = l * w.double().reshape(-1)
    return l.mean()


def test_mmd_cal_dispatches_cl_with_margin_and_criterion():
    from sug_amd.model import mmd
    ls, X, lt, Y = _features()
    Y = 0.8 * X + 0.6 * Y                                         # negative pairs above the margins in use
    for args, margin in (({'NAME': 'CL'}, 0.2), ({'NAME': 'CL', 'MARGIN': 0.0}, 0.0), ({'NAME': 'CL', 'MARGIN': 0.5}, 0.5)):
        v = mmd.mmd_cal(ls, X, lt, Y, args)
        assert v.dim() == 0 and abs(float(v) - float(_by_hand(ls, X, lt, Y, margin))) <= 1e-6
    # the caller's criterion wins over MARGIN
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CL', 'MARGIN': 0.5}, CL_criterion=nn.CosineEmbeddingLoss(margin=-0.3, reduction='none'))
    assert abs(float(v) - float(_by_hand(ls, X, lt, Y, -0.3))) <= 1e-6
    assert abs(float(_by_hand(ls, X, lt, Y, -0.3)) - float(_by_hand(ls, X, lt, Y, 0.5))) > 1e-2
    # any callable criterion takes the composed lines: a lambda sees the plain features and the +-1 targets
    seen = []
    crit = lambda a, b, t: (seen.append((a, b, t)), (a - b).pow(2).sum(1) * t)[1]
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CL'}, CL_criterion=crit)
    t = (2 * (ls == lt).long() - 1)
    assert seen[0][0] is X and seen[0][1] is Y and torch.equal(seen[0][2], t)
    assert torch.equal(v, ((X - Y).pow(2).sum(1) * t).mean())
    # fp64 stays fp64
    assert mmd.mmd_cal(ls, X.double(), lt, Y.double(), {'NAME': 'CL'}).dtype == torch.float64


def test_mmd_cal_weights_cl_by_its_existing_precedence(monkeypatch):
    from sug_amd.model import mmd
    ls, X, lt, Y = _features()
    Y = 0.8 * X + 0.6 * Y
    w_geo, w_sem = torch.rand(1, 6) + 0.5, torch.rand(1, 6) + 0.5
    calls = []
    monkeypatch.setattr(mmd, 'geometric_weights', lambda a, b, weighting='none', KPC=False: (calls.append(('geo', weighting)), w_geo)[1])
    monkeypatch.setattr(mmd, 'prob_weights_soft', lambda a, b, la, lb, lw, weighting='mean2one': (calls.append(('sem', weighting, lw)), w_sem)[1])
    data = torch.zeros(6, 10)
    want = lambda w: float(_by_hand(ls, X, lt, Y, 0.2, w))
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CL', 'GEO_WEIGHTS': 'mean2one'}, data_s=data, data_t=data)
    assert calls == [('geo', 'mean2one')] and abs(float(v) - want(w_geo)) <= 1e-6
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CL', 'SEM_WEIGHTS': 'mean2one', 'LABEL_WEIGHT': 0.5}, data_s=data, data_t=data)
    assert calls[1:] == [('sem', 'mean2one', 0.5)] and abs(float(v) - want(w_sem)) <= 1e-6
    # GEO before SEM (cal_sample_weights), no data -> no weights, given weights are taken as they are
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CL', 'GEO_WEIGHTS': 'none', 'SEM_WEIGHTS': 'mean2one', 'LABEL_WEIGHT': 0.5}, data_s=data,
                    data_t=data)
    assert calls[2:] == [('geo', 'none')] and abs(float(v) - want(w_geo)) <= 1e-6
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CL', 'GEO_WEIGHTS': 'mean2one'})
    assert len(calls) == 3 and abs(float(v) - want(None)) <= 1e-6
    v = mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CL'}, sample_weights=w_sem)
    assert len(calls) == 3 and abs(float(v) - want(w_sem)) <= 1e-6
    assert abs(want(w_geo) - want(w_sem)) > 1e-4 and abs(want(None) - want(w_sem)) > 1e-4


def test_unknown_name_still_raises_and_multi_takes_cl_terms_only():
    from sug_amd.model import mmd
    ls, X, lt, Y = _features()
    with pytest.raises(RuntimeError, match='Not Supported MMD Method'):
        mmd.mmd_cal(ls, X, lt, Y, {'NAME': 'CLX'})
    with pytest.raises(RuntimeError, match='CL terms only'):
        mmd.cl_loss_multi(ls, lt, [(X, Y, {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 1}, None, None)])
    # CPU tensors: term by term through the composed lines, the values of mmd_cal
    terms = [(X, Y, {'NAME': 'CL'}, None, None), (X[:, :3], Y[:, :3], {'NAME': 'CL', 'MARGIN': 0.0}, None, None)]
    vals = mmd.cl_loss_multi(ls, lt, terms)
    for v, (fs, ft, args, _, _) in zip(vals, terms):
        assert torch.equal(v, mmd.mmd_cal(ls, fs, lt, ft, args))


def test_header_ctypes_table_and_python_limits_agree():
    from sug_amd import _lib, ops
    H = _lib.CONSTANTS
    assert (ops.CL_LOSS_MAX_ROWS, ops.CL_LOSS_MAX_D, ops.CL_LOSS_MAX_TERMS) == \
        (H['SUG_CL_LOSS_MAX_ROWS'], H['SUG_CL_LOSS_MAX_D'], H['SUG_CL_LOSS_MAX_TERMS']) == (1024, 1 << 20, 4)
    assert (H['SUG_CL_LOSS_SUM_FIELDS'], H['SUG_CL_LOSS_ROW_FIELDS'], H['SUG_ABI_VERSION']) == (3, 4, 8)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    want = {'sug_cl_loss_fwd': [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
            'sug_cl_loss_bwd': [i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]}
    L = _lib.lib()
    assert L.sug_abi_version() == 8
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == args, name
        assert getattr(L, name).argtypes == args


def _refused(rc, what):
    from sug_amd import _lib
    msg = _lib.lib().sug_last_error().decode()
    assert rc == -1 and re.search(what, msg), (rc, msg)


def test_limits_are_checked_on_the_host_and_name_the_argument():
    """One past each limit: refused before any launch, the message names the entry point, the argument and the limit.  The
    buffers are host memory; nothing reads them."""
    from sug_amd import _lib
    L, H = _lib.lib(), _lib.CONSTANTS
    M, DM, NT = H['SUG_CL_LOSS_MAX_ROWS'], H['SUG_CL_LOSS_MAX_D'], H['SUG_CL_LOSS_MAX_TERMS']
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    P = lambda n, v=p: (ctypes.c_void_p * n)(*[v] * n)
    I64 = lambda n, v: (ctypes.c_int64 * n)(*[v] * n)
    I32 = lambda n, v: (ctypes.c_int32 * n)(*[v] * n)
    F64 = lambda n, v: (ctypes.c_double * n)(*[v] * n)

    def fwd(n=1, m=8, D=8, ld=8, margin=0.2, x=p):
        k = max(n, 1)
        return L.sug_cl_loss_fwd(n, P(k, x), I64(k, ld), P(k), I64(k, ld), I32(k, D), F64(k, margin), p, p, m, P(k, None), p, P(k, None),
                                 p, None)

    for n in (0, NT + 1):
        _refused(fwd(n=n), r'sug_cl_loss_fwd: %d terms \(1\.\.%d\)' % (n, NT))
    for m in (0, M + 1):
        _refused(fwd(m=m), r'sug_cl_loss_fwd: m=%d\b.*\b%d\b' % (m, M))
    for D in (0, DM + 1):
        _refused(fwd(D=D, ld=DM + 1), r'sug_cl_loss_fwd: D=%d\b.*\b%d\b' % (D, DM))
    _refused(fwd(ld=7), r'sug_cl_loss_fwd: row stride 7 < D=8')
    for margin in (float('nan'), float('inf')):
        _refused(fwd(margin=margin), r'sug_cl_loss_fwd: margin of term 0 is not finite')
    _refused(fwd(x=None), r'sug_cl_loss_fwd: null feature pointer of term 0')
    _refused(L.sug_cl_loss_fwd(1, P(1), I64(1, 8), P(1), I64(1, 8), I32(1, 8), F64(1, 0.2), None, p, 8, P(1, None), p, P(1, None), p,
                               None), r'sug_cl_loss_fwd: null pointer')

    def bwd(n=1, m=8, D=8, ld=8, ldd=8, coef=p):
        k = max(n, 1)
        return L.sug_cl_loss_bwd(n, P(k), I64(k, ld), P(k), I64(k, ld), I32(k, D), m, P(k, coef), P(k), P(k), I64(k, ldd), P(k),
                                 I64(k, ldd), None)

    _refused(bwd(n=NT + 1), r'sug_cl_loss_bwd: %d terms' % (NT + 1))
    _refused(bwd(m=M + 1), r'sug_cl_loss_bwd: m=%d\b' % (M + 1))
    _refused(bwd(D=DM + 1, ld=DM + 1, ldd=DM + 1), r'sug_cl_loss_bwd: D=%d\b' % (DM + 1))
    _refused(bwd(ld=7), r'sug_cl_loss_bwd: row stride 7 < D=8')
    _refused(bwd(ldd=7), r'sug_cl_loss_bwd: gradient row stride < D=8')
    _refused(bwd(coef=None), r'sug_cl_loss_bwd: null coefficients of term 0')


def test_cl_loss_supported_refuses_what_the_kernels_do_not_take(monkeypatch):
    from sug_amd import ops
    ls, X, lt, Y = _features()
    assert not ops.cl_loss_supported(ls, X, lt, Y)                              # CPU tensors
    # the remaining rules do not depend on where the tensors live: a stand-in that says 'HIP device'
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    assert ops.cl_loss_supported(ls, X, lt, Y) and ops.cl_loss_supported(ls, X, lt, Y, 0.5, torch.ones(1, 6))
    assert not ops.cl_loss_supported(ls, X.double(), lt, Y.double())            # fp64
    assert not ops.cl_loss_supported(ls, X, lt, Y[:, :4])                       # mismatched shapes
    assert not ops.cl_loss_supported(ls, X[:5], lt, Y[:5])                      # labels of another length
    assert not ops.cl_loss_supported(ls.int(), X, lt.int(), Y)                  # int32 labels
    assert not ops.cl_loss_supported(ls.reshape(-1, 1), X, lt.reshape(-1, 1), Y)
    assert not ops.cl_loss_supported(ls, X[0], lt, Y[0])                        # 1-D features
    assert not ops.cl_loss_supported(ls, X, lt, Y, float('nan'))
    assert not ops.cl_loss_supported(ls, X, lt, Y, 0.2, torch.ones(1, 6, requires_grad=True))
    assert not ops.cl_loss_supported(ls, X, lt, Y, 0.2, torch.ones(5))
    big_m = ops.CL_LOSS_MAX_ROWS + 1
    lab = torch.zeros(big_m, dtype=torch.int64)
    assert not ops.cl_loss_supported(lab, torch.zeros(big_m, 2), lab, torch.zeros(big_m, 2))
    assert ops.cl_loss_supported(lab[:-1], torch.zeros(big_m - 1, 2), lab[:-1], torch.zeros(big_m - 1, 2))
    wide = torch.zeros(1, 1).expand(1, ops.CL_LOSS_MAX_D + 1)                   # no memory behind it
    assert not ops.cl_loss_supported(lab[:1], wide, lab[:1], wide)
    assert ops.cl_loss_supported(lab[:1], wide[:, :-1], lab[:1], wide[:, :-1])
    monkeypatch.setattr(ops, 'CL_LOSS', False)                                  # SUG_CL_LOSS=0
    assert not ops.cl_loss_supported(ls, X, lt, Y)


def test_cpu_tensors_are_refused_by_the_op_and_take_the_composed_lines_in_the_mirror():
    from sug_amd import ops
    from sug_amd.model import mmd
    ls, X, lt, Y = _features()
    with pytest.raises(RuntimeError):
        ops.cl_loss(ls, X, lt, Y)
    v = mmd.contrastive_loss_weighted(ls, X, lt, Y, 0.3, nn.CosineEmbeddingLoss(margin=0.2, reduction='none'))
    assert abs(float(v) - float(_by_hand(ls, X, lt, Y, 0.2))) <= 1e-6
    # label_weight takes no part in the value
    assert torch.equal(v, mmd.contrastive_loss_weighted(ls, X, lt, Y, 7.0, nn.CosineEmbeddingLoss(margin=0.2, reduction='none')))
