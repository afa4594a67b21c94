"""GPU: the BatchNorm row and pooling kernels on every dispatch path (tests/bn_paths_cases.py: the float4 and the scalar
column reduction with 1 .. 16 channel trips, grouped launches up to 16 groups and each of their refusals -- more than 16
groups, more partial rows than the workspace holds, a scalar layout -- rows per workgroup past 4 ly, eval mode with and
without groups, a misaligned or padded gradient, the pre=(out, coef) form; the pooling kernels with N < 4, partial channel
blocks, the three apply kernels, padded and misaligned y, B at and past the workspace limit, exact ties) through the public
ops under ops.bn_groups, against the fp64 restatement under the project's bound: per tensor err(kernel) <= 8
err(fp32 torch) + 1e-7.  Each tensor's two figures are printed as `bn-paths-ratio <case> <tensor> <err kernel> <err fp32>`
before the assertion (profiles/bn_paths_fp64_ratios.txt).  Before a case runs, the path it takes is asserted from the
library's answer (ops.bn_rows_plan); it runs twice with equal bits, and with G > 1 it is held bit for bit against G separate
calls on the groups' rows.

rows/c1 found a bug: col_reduce_kernel folded its up to 256 row-lanes serially in fp32, dgamma of the case came out 7.2e-7 of
itself off against 1.5e-8 of fp32 torch (bound 2.2e-7); the fold is in fp64 now."""
import pytest
import torch

import bn_paths_cases as P

pytestmark = pytest.mark.gpu


def _module(c, train):
    bn = torch.nn.BatchNorm1d(c['C'], eps=P.EPS, momentum=P.MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(c['gamma']), bn.bias.copy_(c['beta']), bn.running_mean.copy_(c['mean']), bn.running_var.copy_(c['var'])
    return bn.cuda().train(train)


def _column_slice(t, off, width):
    """t [..., C] as the columns off .. off + C of a wider device tensor filled with other numbers."""
    C = t.shape[-1]
    wide = torch.full(t.shape[:-1] + (C + width,), 7.0)
    wide[..., off:off + C] = t
    v = wide.cuda()[..., off:off + C]
    assert v.stride(-1) == 1 and v.stride(-2) == C + width and (v.data_ptr() % 16 == 0) == (off % 4 == 0)
    return v


def _bound(label, got, r64, r32, names):
    errs = {t: (P.err(got[t], r64[t]), P.err(r32[t], r64[t])) for t in names}
    for t, (ek, e32) in errs.items():
        print('bn-paths-ratio %s %s %.4g %.4g' % (label, t, ek, e32))
    for t in names:
        assert tuple(got[t].shape) == tuple(r64[t].shape) and bool(torch.isfinite(got[t]).all()), (label, t)
    bad = {t: v for t, v in errs.items() if not P.within(*v)}
    assert not bad, '%s: err(kernel), err(fp32 torch) = %r' % (label, bad)


def _same_bits(a, b, names, label):
    for t in names:
        assert torch.equal(a[t], b[t]), (label, t)


def _fold_close(whole, parts):
    """dgamma / dbeta of a grouped call = fp32(sum of the groups' fp64 sums); separate calls round each group's sum to fp32
    first: the two differ by the roundings of the parts and of the total, half an ulp each."""
    total = torch.stack([p.double() for p in parts]).sum(dim=0)
    slack = 2.0 ** -23 * (torch.stack([p.double().abs() for p in parts]).sum(dim=0) + whole.double().abs())
    return bool(((whole.double() - total).abs() <= slack).all())


# ----------------------------------------------------------------------------- ops.bn_act_rows
def _assert_rows_path(name):
    from sug_amd import ops
    s, e = P.rows_shape(name), P.ROWS_EXPECT[name]
    rg, C, G = s['rows'] // s['G'], s['C'], s['G']
    gs = s['opt'].get('gslice')
    assert P.rows_case_path(name)[:2] == (e['fwd'], e['bwd'])
    if s['train']:
        assert ops.bn_rows_plan(rg, C, C, G, False, 0, True) == e['plan'], name
    mode = 2 if s['train'] and e['bplan'][0] else 1
    assert ops.bn_rows_plan(rg, C, C + P.GWIDE if gs else C, G, False, mode, gs != 'mis') == e['bplan'], name


def _run_rows(name, lo=None, hi=None, bn=None, groups=None):
    """One forward + backward of the case (of its rows lo .. hi as a call of their own, on the module bn) -> the compared
    tensors on the CPU."""
    from sug_amd import ops
    c = P.rows_inputs(name)
    C, train, opt = c['C'], c['train'], c['opt']
    G = c['G'] if groups is None else groups
    bn = _module(c, train) if bn is None else bn
    bn.weight.grad = bn.bias.grad = None
    sl = slice(lo, hi)
    y = c['y'][sl].clone()
    if 'shape' in opt and lo is None:
        y = y.view(opt['shape'])
    y = y.cuda().requires_grad_(True)
    gout = P.rows_probe(name)[0][sl]
    gs = opt.get('gslice')
    g = _column_slice(gout, 1 if gs == 'mis' else 4, P.GWIDE) if gs else gout.cuda()
    with ops.bn_groups(G):
        out = ops.bn_act_rows(y, bn, c['slope'])
    assert tuple(out.shape) == tuple(y.shape) and y.data_ptr() % 16 == 0
    out.backward(g.view(out.shape) if not gs else g)
    torch.cuda.synchronize()
    return {'out': out.detach().reshape(-1, C).cpu(), 'dy': y.grad.reshape(-1, C).cpu(), 'dgamma': bn.weight.grad.cpu().clone(),
            'dbeta': bn.bias.grad.cpu().clone(), 'mean': bn.running_mean.cpu().clone(), 'var': bn.running_var.cpu().clone(),
            'count': int(bn.num_batches_tracked)}


ROWS_BITS = ('out', 'dy', 'dgamma', 'dbeta', 'mean', 'var')


@pytest.mark.parametrize('name', sorted(n for n in P.ROWS_CASES if not P.rows_shape(n)['opt'].get('pre')))
def test_bn_act_rows_path_against_fp64_twice_the_same_bits_and_as_separate_calls(name):
    c = P.rows_inputs(name)
    G, train, rg, C = c['G'], c['train'], c['rows'] // c['G'], c['C']
    _assert_rows_path(name)
    got = _run_rows(name)
    _bound('rows/' + name, got, P.rows_reference(name, 'float64'), P.rows_reference(name, 'float32'), P.rows_compared(name))
    assert got['count'] == (G if train else 0)
    if not train:                                      # eval mode leaves the running buffers alone
        assert torch.equal(got['mean'], c['mean']) and torch.equal(got['var'], c['var'])
    again = _run_rows(name)
    _same_bits(got, again, ROWS_BITS, name)
    if G > 1:
        bn = _module(c, train)
        parts = [_run_rows(name, i * rg, (i + 1) * rg, bn, groups=1) for i in range(G)]
        assert parts[-1]['count'] == (G if train else 0)
        # the grouped launch shares one workspace among the groups: where that makes it cut a group into other workgroups
        # than a call of its own would (include/sug_amd.h, sug_col_stats_bn_grouped), the fp32 partial sums differ
        single_f, single_b = P.col_plan(rg, C), P.col_plan(rg, C, mode=1)
        e = P.ROWS_EXPECT[name]
        same_cut = (not train or e['plan'][3] < 0 or e['plan'][2] == single_f[2]) and \
                   (e['bplan'][3] < 0 or not e['bplan'][0] or e['bplan'][2] == single_b[2])
        assert same_cut == (name != 'rpb-g2')
        sep = {'out': torch.cat([p['out'] for p in parts]), 'dy': torch.cat([p['dy'] for p in parts]), 'mean': parts[-1]['mean'],
               'var': parts[-1]['var']}
        if same_cut:
            _same_bits(got, sep, ('out', 'dy', 'mean', 'var'), name + ' grouped vs separate')
        else:                                          # both sides stand under the bar
            sep.update(dgamma=sum(p['dgamma'].double() for p in parts).float(), dbeta=sum(p['dbeta'].double() for p in parts).float())
            _bound('rows/' + name + '/separate', sep, P.rows_reference(name, 'float64'), P.rows_reference(name, 'float32'),
                   P.rows_compared(name))
        if same_cut:
            for t in ('dgamma', 'dbeta'):
                assert _fold_close(got[t], [p[t] for p in parts]), (name, t)


def test_bn_act_rows_pre_launches_nothing_and_gives_the_case_its_own_backward():
    from sug_amd import ops
    name = 'pre'
    c = P.rows_inputs(name)
    _assert_rows_path(name)
    first = _run_rows(name)
    bn = _module(c, True)
    y = c['y'].cuda().requires_grad_(True)
    with ops.bn_groups(c['G']), ops.record_bn_stats() as rec:
        out = ops.bn_act_rows(y, bn, c['slope'])
    (_, coef), = rec
    assert tuple(coef.shape) == (c['G'], 5, c['C'])
    mean, var, count = bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)
    assert count == c['G'] and torch.equal(mean.cpu(), first['mean'])
    y2 = c['y'].cuda().requires_grad_(True)
    with ops.bn_groups(c['G']), ops.record_bn_stats() as rec2:
        out2 = ops.bn_act_rows(y2, bn, c['slope'], pre=(out.detach(), coef))
    assert rec2 == [] and out2.data_ptr() == out.data_ptr()          # nothing recorded, nothing written: the earlier pass's tensor
    assert torch.equal(bn.running_mean, mean) and torch.equal(bn.running_var, var) and int(bn.num_batches_tracked) == count
    out2.backward(P.rows_probe(name)[0].cuda())
    got = {'out': out2.detach().cpu(), 'dy': y2.grad.cpu(), 'dgamma': bn.weight.grad.cpu(), 'dbeta': bn.bias.grad.cpu(),
           'mean': bn.running_mean.cpu(), 'var': bn.running_var.cpu()}
    _same_bits(got, first, ROWS_BITS, name)
    _bound('rows/pre', got, P.rows_reference(name, 'float64'), P.rows_reference(name, 'float32'), P.rows_compared(name))


# ----------------------------------------------------------------------------- ops.bn_act_pool_cat
def _assert_pool_path(name, grouped):
    from sug_amd import ops
    s, e = P.pool_shape(name), P.POOL_EXPECT[name]
    B, N, C, G = s['B'], s['N'], s['C'], s['G']
    ys = s['opt'].get('yslice')
    fwd, bwd, ap, plan = P.pool_case_path(name, grouped)
    if grouped:
        assert (fwd, bwd, ap, plan) == (e['fwd'], e['bwd'], e['apply'], e['plan'])
    else:
        assert (fwd, bwd) == ('loop', 'loop')
    if s['train']:
        tryg = grouped and 1 < G <= P.MAX_GROUPS
        assert ops.bn_rows_plan(B // G * N, C, C + 4 if ys else C, G if tryg else 1, tryg, 0, ys != 'mis') == plan, name


def _run_pool(name, lo=None, hi=None, bn=None, groups=None, grouped=None):
    from sug_amd import ops
    c = P.pool_inputs(name)
    C, train, opt = c['C'], c['train'], c['opt']
    G = c['G'] if groups is None else groups
    bn = _module(c, train) if bn is None else bn
    bn.weight.grad = bn.bias.grad = None
    sl = slice(lo, hi)
    ys = opt.get('yslice')
    y = (_column_slice(c['y'][sl], 1 if ys == 'mis' else 4, 4) if ys else c['y'][sl].clone().cuda()).requires_grad_(True)
    g = _column_slice(c['gout'][sl], 4, 8) if opt.get('gslice') else c['gout'][sl].cuda()
    keep = ops.BN_POOL_GROUPED
    try:
        if grouped is not None:
            ops.BN_POOL_GROUPED = grouped
        with ops.bn_groups(G):
            pooled = ops.bn_act_pool_cat(y, bn, c['slope'])
        assert tuple(pooled.shape) == (y.shape[0], 2 * C)
        if opt.get('refused'):
            with pytest.raises(RuntimeError, match='bad shape'):
                pooled.backward(g)
            dy = dg = db = None
        else:
            pooled.backward(g)
            dy, dg, db = y.grad.cpu(), bn.weight.grad.cpu().clone(), bn.bias.grad.cpu().clone()
    finally:
        ops.BN_POOL_GROUPED = keep
    torch.cuda.synchronize()
    return {'max': pooled.detach()[:, :C].cpu(), 'mean_n': pooled.detach()[:, C:].cpu(), 'dy': dy, 'dgamma': dg, 'dbeta': db,
            'mean': bn.running_mean.cpu().clone(), 'var': bn.running_var.cpu().clone(), 'count': int(bn.num_batches_tracked)}


@pytest.mark.parametrize('name', sorted(P.POOL_CASES))
def test_bn_act_pool_path_against_fp64_twice_the_same_bits_and_as_separate_calls(name):
    from sug_amd import ops
    c = P.pool_inputs(name)
    G, train, Bg = c['G'], c['train'], c['B'] // c['G']
    assert ops.BN_POOL_GROUPED                          # as shipped
    _assert_pool_path(name, True)
    got = _run_pool(name)
    names = [t for t in P.pool_compared(name) if got[t] is not None]
    assert len(names) == len(P.pool_compared(name)) - (3 if c['opt'].get('refused') else 0)
    _bound('pool/' + name, got, P.pool_reference(name, 'float64'), P.pool_reference(name, 'float32'), names)
    assert got['count'] == (G if train else 0)
    if not train:
        assert torch.equal(got['mean'], c['mean']) and torch.equal(got['var'], c['var'])
    bits = [t for t in ('max', 'mean_n', 'dy', 'dgamma', 'dbeta', 'mean', 'var') if got[t] is not None]
    _same_bits(got, _run_pool(name), bits, name)
    if G > 1:
        _assert_pool_path(name, False)
        _same_bits(got, _run_pool(name, grouped=False), bits, name + ' BN_POOL_GROUPED = False')
        bn = _module(c, train)
        parts = [_run_pool(name, i * Bg, (i + 1) * Bg, bn, groups=1) for i in range(G)]
        assert parts[-1]['count'] == (G if train else 0)
        sep = {t: torch.cat([p[t] for p in parts]) for t in ('max', 'mean_n', 'dy')}
        sep.update(mean=parts[-1]['mean'], var=parts[-1]['var'])
        _same_bits(got, sep, ('max', 'mean_n', 'dy', 'mean', 'var'), name + ' grouped vs separate')
        for t in ('dgamma', 'dbeta'):
            assert _fold_close(got[t], [p[t] for p in parts]), (name, t)


# ----------------------------------------------------------------------------- the statistics ops
def _layout(t, lay):
    return t.clone().cuda() if lay == 'dense' else _column_slice(t, 4 if lay == 'pad' else 1, P.SWIDE)


def _buffers(bn):
    return {'mean': bn.running_mean.cpu().clone(), 'var': bn.running_var.cpu().clone(), 'count': int(bn.num_batches_tracked)}


def _assert_stats_path(name):
    from sug_amd import ops
    op, rows, C, G, lay = P.STATS_CASES[name]
    how, plan = P.STATS_EXPECT[name]
    assert P.stats_expect(name) == (how, plan)
    if plan is not None:
        ld, al = (C, True) if lay == 'dense' else (C + P.SWIDE, lay == 'pad')
        tryg = op == 'update' and 1 < G <= P.MAX_GROUPS
        assert ops.bn_rows_plan(rows // G, C, ld, G if tryg else 1, tryg, 0, al) == plan, name


def _recurrence_refs(c):
    refs = []
    for dt in (torch.float64, torch.float32):
        m, _, u = P.moments(c['y'].to(dt), c['G'])
        rm, rv = P.recurrence(c['mean'].to(dt), c['var'].to(dt), m, u)
        refs.append({'mean': rm, 'var': rv})
    return refs


@pytest.mark.parametrize('name', sorted(n for n in P.STATS_CASES if P.STATS_CASES[n][0] == 'update'))
def test_bn_update_stats_path_against_fp64_and_as_separate_calls(name):
    from sug_amd import ops
    c = P.stats_inputs(name)
    G, rg = c['G'], c['rows'] // c['G']
    _assert_stats_path(name)

    def run(grouped=None, train=True):
        bn = _module(c, train)
        keep = ops.BN_POOL_GROUPED
        try:
            if grouped is not None:
                ops.BN_POOL_GROUPED = grouped
            with ops.bn_groups(G):
                ops.bn_update_stats(_layout(c['y'], c['lay']), bn)
        finally:
            ops.BN_POOL_GROUPED = keep
        return _buffers(bn)

    got = run()
    r64, r32 = _recurrence_refs(c)
    _bound('stats/' + name, got, r64, r32, ('mean', 'var'))
    assert got['count'] == G
    _same_bits(got, run(), ('mean', 'var'), name)
    idle = run(train=False)                             # eval mode: no update
    assert torch.equal(idle['mean'], c['mean']) and torch.equal(idle['var'], c['var']) and idle['count'] == 0
    if G > 1:
        _same_bits(got, run(grouped=False), ('mean', 'var'), name + ' BN_POOL_GROUPED = False')
        bn = _module(c, True)
        for i in range(G):
            ops.bn_update_stats(_layout(c['y'][i * rg:(i + 1) * rg], c['lay']), bn)
        sep = _buffers(bn)
        _same_bits(got, sep, ('mean', 'var'), name + ' grouped vs separate')
        assert sep['count'] == G


@pytest.mark.parametrize('name', ['col-stats-pad', 'col-stats-mis'])
def test_col_stats_against_fp64(name):
    from sug_amd import ops
    c = P.stats_inputs(name)
    _assert_stats_path(name)
    y = _layout(c['y'], c['lay'])
    s = ops.col_stats(y)
    C = c['C']
    assert s.dtype == torch.float64 and tuple(s.shape) == (2 * C,)
    refs = [{'sum': c['y'].to(dt).sum(dim=0), 'sumsq': c['y'].to(dt).pow(2).sum(dim=0)} for dt in (torch.float64, torch.float32)]
    _bound('stats/' + name, {'sum': s[:C].cpu(), 'sumsq': s[C:].cpu()}, refs[0], refs[1], ('sum', 'sumsq'))
    assert torch.equal(ops.col_stats(y), s)


@pytest.mark.parametrize('name', ['affine-pad', 'affine-mis'])
def test_affine_act_into_a_padded_out_against_fp64(name):
    from sug_amd import ops
    c = P.stats_inputs(name)
    C, off = c['C'], 4 if c['lay'] == 'pad' else 1
    coef = P.coef_rows(c, c['y'], torch.float32)[0].contiguous()          # the fp32 coefficients are the op's input
    wide = torch.full((c['rows'], C + P.SWIDE), 7.0).cuda()
    out = wide[:, off:off + C]
    res = ops.affine_act(c['y'].cuda(), coef.cuda(), c['slope'], out=out)
    assert res.data_ptr() == out.data_ptr()
    refs = [{'out': P.act(c['y'].to(dt) * coef[0].to(dt) + coef[1].to(dt), c['slope'])} for dt in (torch.float64, torch.float32)]
    _bound('stats/' + name, {'out': out.cpu()}, refs[0], refs[1], ('out',))
    keep = torch.ones(C + P.SWIDE, dtype=torch.bool)
    keep[off:off + C] = False
    assert bool((wide.cpu()[:, keep] == 7.0).all())                        # the padding is not written


def test_bn_coef_against_fp64():
    from sug_amd import ops
    name = 'coef'
    c = P.stats_inputs(name)
    C, rows = c['C'], c['rows']
    y64 = c['y'].double()
    stats = torch.cat((y64.sum(dim=0), y64.pow(2).sum(dim=0))).cuda()
    bn = _module(c, True)
    coef = ops.bn_coef(stats, bn.weight.detach(), bn.bias.detach(), rows, P.EPS, P.MOMENTUM, bn.running_mean, bn.running_var)
    rows5 = ('scale', 'shift', 'bmean', 'rstd', 'unbiased')
    got = dict(zip(rows5, coef.cpu()), mean=bn.running_mean.cpu(), var=bn.running_var.cpu())
    refs = []
    for (r, k) in zip(_recurrence_refs(c), (P.coef_rows(c, c['y'], torch.float64)[0], P.coef_rows(c, c['y'], torch.float32)[0])):
        refs.append(dict(zip(rows5, k), **r))
    _bound('stats/' + name, got, refs[0], refs[1], rows5 + ('mean', 'var'))


@pytest.mark.parametrize('name', ['replay', 'replay-g17'])
def test_bn_replay_gives_the_buffers_the_forward_left(name):
    from sug_amd import ops
    c = P.stats_inputs(name)
    G = c['G']
    bn = _module(c, True)
    with ops.bn_groups(G), ops.record_bn_stats() as rec:
        ops.bn_act_rows(c['y'].cuda(), bn, c['slope'])
    (_, coef), = rec
    assert tuple(coef.shape) == (G, 5, c['C'])
    left = _buffers(bn)
    bn2 = _module(c, True)
    ops.bn_replay(bn2, coef)
    got = _buffers(bn2)
    assert got['count'] == G == left['count']
    _same_bits(got, left, ('mean', 'var'), name)
    r64, r32 = _recurrence_refs(c)
    _bound('stats/' + name, got, r64, r32, ('mean', 'var'))
    k64, k32 = P.coef_rows(c, c['y'], torch.float64), P.coef_rows(c, c['y'], torch.float32)
    _bound('stats/' + name + '/coef', {'coef': coef.cpu()}, {'coef': k64}, {'coef': k32}, ('coef',))
