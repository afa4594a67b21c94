"""CPU checks of tests/bn_paths_cases.py: the tables hold every regime of the BatchNorm row and pooling dispatch, each probe
zeroes few entries, the fp32 torch form keeps the margins for the chosen seed (where the probe is live it stands on the fp64
form's side of the kink and picks the same row), the restatements equal F.batch_norm + F.leaky_relu + max / mean in fp64,
the tie cases route to the row the kernels' rule names, and every case reaches what its EXPECT entry says -- by the launch
arithmetic restated in the cases module and by the library's own answer (ops.bn_rows_plan: host-side, no launch)."""
import pytest
import torch

import bn_paths_cases as P

ROWS, POOL, STATS = sorted(P.ROWS_CASES), sorted(P.POOL_CASES), sorted(P.STATS_CASES)
TIE_FREE_POOL = [n for n in POOL if 'tie' not in P.pool_shape(n)['opt']]


def test_the_tables_are_the_ones_the_paths_need():
    assert set(P.ROWS_EXPECT) == set(P.ROWS_CASES) and set(P.POOL_EXPECT) == set(P.POOL_CASES) and set(P.STATS_EXPECT) == set(P.STATS_CASES)
    R, S = P.ROWS_EXPECT, {n: P.rows_shape(n) for n in ROWS}
    for n in ROWS:
        assert S[n]['rows'] % S[n]['G'] == 0 and 1 <= S[n]['C'] <= 4096 and S[n]['rows'] * S[n]['C'] <= 5 << 20, n
    assert {R[n]['fwd'] for n in ROWS} >= {'vec', 'scalar', 'grouped', 'refused-groups', 'refused-grid', 'refused-scalar', 'eval',
                                          'eval-grouped', 'eval-loop'}
    # 'mode1-grouped' (a train-mode grouped MODE 1 reduce + bn_bwd_apply_vec4_groups_kernel<false>) needs a layout the MODE 2
    # branch refuses and the MODE 1 launch takes; with the dense, aligned y / dy of ops.bn_act_rows there is none
    assert {R[n]['bwd'] for n in ROWS} == {'mode2', 'loop-vec', 'loop-scalar', 'eval-grouped', 'eval-loop-vec', 'eval-loop-scalar'}
    assert {S[n]['slope'] for n in ROWS} == {0.0, 0.01, 0.2, 1.0} and {S[n]['G'] for n in ROWS} >= {1, 2, 16, 17}
    assert {S[n]['C'] for n in ROWS} >= {1, 3, 7, 8, 70, 1028, 4095, 4096}
    assert {R[n]['trips'] for n in ROWS} >= {1, 2, 4, 16}
    for G in (1, 2):
        assert any(S[n]['G'] == G and R[n]['plan'] and R[n]['plan'][0] and R[n]['plan'][2] > 4 * (256 // R[n]['plan'][1]) for n in ROWS), G
        assert any(S[n]['G'] == G and S[n]['C'] == 70 for n in ROWS)
        assert {S[n]['opt'].get('gslice') for n in ROWS if S[n]['G'] == G} >= {'mis', 'pad'}
        assert any(S[n]['G'] == G and not S[n]['train'] and S[n]['C'] % 4 == 0 for n in ROWS)
    assert any(S[n]['G'] == 2 and not S[n]['train'] and S[n]['C'] % 4 for n in ROWS)
    assert any(S[n]['rows'] // S[n]['G'] == 2 and S[n]['C'] == 8 for n in ROWS)
    assert any(len(S[n]['opt'].get('shape', ())) == 4 for n in ROWS) and any(S[n]['opt'].get('pre') for n in ROWS)

    E, Q = P.POOL_EXPECT, {n: P.pool_shape(n) for n in POOL}
    assert {Q[n]['C'] for n in POOL} >= {4, 24, 64, 70, 100, 2048} and {Q[n]['N'] for n in POOL} >= {1, 2, 3, 5, 67, 300}
    assert {Q[n]['G'] for n in POOL} >= {1, 2, 16, 17} and {Q[n]['B'] for n in POOL} >= {256, 257}
    assert {(E[n]['fwd'], E[n]['bwd']) for n in POOL} >= {('loop', 'loop'), ('grouped', 'grouped'), ('grouped', 'loop'), ('loop', 'refused')}
    assert {E[n]['apply'] for n in POOL} == {'rows', 'vec4', 'scalar'}
    assert {(Q[n]['C'], Q[n]['G']) for n in POOL} >= {(64, 1), (64, 2), (70, 1), (70, 2)}
    assert {Q[n]['G'] for n in POOL if not Q[n]['train']} >= {1, 2}
    assert {Q[n]['opt'].get('yslice') for n in POOL} >= {'pad', 'mis'} and any(Q[n]['opt'].get('gslice') for n in POOL)
    assert {Q[n]['opt'].get('tie') for n in POOL} >= {'chunk', 'lane', 'first', 'const'}
    for n in POOL:
        assert Q[n]['B'] % Q[n]['G'] == 0 and Q[n]['B'] // Q[n]['G'] * Q[n]['N'] >= 2, n
    (n1, n2), chunk = P.TIE_ROWS['chunk'], lambda n: [b for b in range(4) if 67 * b // 4 <= n < 67 * (b + 1) // 4][0]
    assert chunk(n1) != chunk(n2) and n1 < n2
    for kind, same_lane in (('lane', False), ('first', True)):
        n1, n2 = P.TIE_ROWS[kind]
        assert chunk(n1) == chunk(n2) and n1 < n2 and ((n1 - n2) % 16 == 0) == same_lane

    T = {n: P.STATS_CASES[n] for n in STATS}
    assert {(T[n][3], T[n][4]) for n in STATS if T[n][0] == 'update'} == {(G, l) for G in (1, 2, 16, 17) for l in ('dense', 'pad', 'mis')}
    assert {T[n][0] for n in STATS} == {'update', 'col_stats', 'affine', 'coef', 'replay'}
    assert {P.STATS_EXPECT[n][0] for n in STATS} == {'grouped', 'loop', 'single', None}


# ----------------------------------------------------------------------------- the paths
def _lib_plan(rows, C, ld, groups, own_ws, mode, aligned):
    from sug_amd import ops
    return ops.bn_rows_plan(rows, C, ld, groups, own_ws, mode, aligned)


@pytest.mark.parametrize('name', ROWS)
def test_rows_case_reaches_what_expect_says(name):
    s, e = P.rows_shape(name), P.ROWS_EXPECT[name]
    fwd, bwd, pf, pb = P.rows_case_path(name)
    assert (fwd, bwd, pf, pb) == (e['fwd'], e['bwd'], e['plan'], e['bplan']), name
    rg, C, G = s['rows'] // s['G'], s['C'], s['G']
    gs = s['opt'].get('gslice')
    ldg, gal = (C + P.GWIDE if gs else C), gs != 'mis'
    if s['train']:
        assert _lib_plan(rg, C, C, G, False, 0, True) == e['plan']
        assert P.trips(C, e['plan']) == e['trips']
        if e['plan'][3] < 0:                                      # the per-group calls that follow the refusal are launched
            assert _lib_plan(rg, C, C, 1, False, 0, True)[3] >= 1
    mode = 2 if bwd == 'mode2' or (s['train'] and e['bplan'][0]) else 1
    assert _lib_plan(rg, C, ldg, G, False, mode, gal) == e['bplan']
    if e['bplan'][3] < 0 or bwd.endswith(('loop-vec', 'loop-scalar')):
        one = _lib_plan(rg, C, ldg, 1, False, 1, gal)
        assert one[3] >= 1 and one[0] == bwd.endswith('vec')


@pytest.mark.parametrize('name', POOL)
def test_pool_case_reaches_what_expect_says(name):
    s, e = P.pool_shape(name), P.POOL_EXPECT[name]
    fwd, bwd, ap, plan = P.pool_case_path(name)
    assert (fwd, bwd, ap, plan) == (e['fwd'], e['bwd'], e['apply'], e['plan']), name
    assert bool(s['opt'].get('refused')) == (bwd == 'refused')
    B, N, C, G = s['B'], s['N'], s['C'], s['G']
    ys = s['opt'].get('yslice')
    ld, al = (C + 4 if ys else C), ys != 'mis'
    if s['train']:
        tryg = 1 < G <= P.MAX_GROUPS
        assert _lib_plan(B // G * N, C, ld, G if tryg else 1, tryg, 0, al) == e['plan']
    if G > 1:                                                     # ops.BN_POOL_GROUPED = False: group by group both ways
        f2, b2, a2, p2 = P.pool_case_path(name, grouped=False)
        assert (f2, b2, a2) == ('loop', 'loop', ap)
        if s['train']:
            assert _lib_plan(B // G * N, C, ld, 1, False, 0, al) == p2 and p2[3] >= 1


@pytest.mark.parametrize('name', STATS)
def test_stats_case_reaches_what_expect_says(name):
    op, rows, C, G, lay = P.STATS_CASES[name]
    how, plan = P.stats_expect(name)
    assert (how, plan) == P.STATS_EXPECT[name]
    if plan is not None:
        ld, al = (C, True) if lay == 'dense' else (C + P.SWIDE, lay == 'pad')
        tryg = op == 'update' and 1 < G <= P.MAX_GROUPS
        assert _lib_plan(rows // G, C, ld, G if tryg else 1, tryg, 0, al) == plan


def test_plan_query_edges():
    """ops.bn_rows_plan on both sides of each term of launch_col_reduce, against the restated arithmetic."""
    from sug_amd import ops
    for rg in (504, 505, 508, 509):                               # G = 16, C = 512: rpb 8, grid 64 from 505 rows on; rpb 10 from 509
        want = P.col_plan(rg, 512, 512, 16)
        assert ops.bn_rows_plan(rg, 512, 512, 16) == want and (want[3] < 0) == (505 <= rg <= 508), (rg, want)
    for rg in (252, 253, 254, 255):                               # C = 1024: the same at 253 .. 254
        want = P.col_plan(rg, 1024, 1024, 16)
        assert ops.bn_rows_plan(rg, 1024, 1024, 16) == want and (want[3] < 0) == (253 <= rg <= 254), (rg, want)
    assert ops.bn_rows_plan(506, 512, 512, 16, own_ws=True) == (True, 128, 8, 64)          # a workspace block per group
    assert ops.bn_rows_plan(40, 32, 32, 16)[3] == 1 and ops.bn_rows_plan(40, 32, 32, 17)[3] == -1
    assert ops.bn_rows_plan(4064, 1024)[2] == 4 and ops.bn_rows_plan(4065, 1024)[2] == 5
    assert ops.bn_rows_plan(300, 64, 68) == (True, 16, 64, 5) and ops.bn_rows_plan(300, 64, 70)[0] is False
    assert ops.bn_rows_plan(300, 64, aligned=False) == (False, 64, 256, 2)
    assert ops.bn_rows_plan(300, 70, mode=1)[3] == 2 and ops.bn_rows_plan(300, 70, mode=2)[3] == -1
    assert ops.bn_rows_plan(300, 70, groups=2)[3] == -1
    assert ops.bn_rows_plan(1 << 22, 3) == P.col_plan(1 << 22, 3) == (False, 4, 8192, 512)          # the scalar rpb doubles
    for C in (1, 2, 3, 4, 7, 8, 70, 100, 1024, 1028, 4095, 4096):
        for rows in (1, 2, 300, 5000):
            for G in (1, 2, 16):
                for mode in (0, 1, 2):
                    for own in (False, True):
                        assert ops.bn_rows_plan(rows, C, C, G, own, mode) == P.col_plan(rows, C, C, G, own, mode), (C, rows, G, mode, own)
    for bad in ((0, 8), (8, 0), (8, 4097)):
        with pytest.raises(RuntimeError, match='sug_bn_rows_plan'):
            ops.bn_rows_plan(*bad)
    with pytest.raises(RuntimeError, match='sug_bn_rows_plan'):
        ops.bn_rows_plan(8, 8, 4)


# ----------------------------------------------------------------------------- the inputs and the margins
@pytest.mark.parametrize('name', ROWS)
def test_rows_inputs_and_probe(name):
    c = P.rows_inputs(name)
    rg, C = c['rows'] // c['G'], c['C']
    assert 1 <= c['dom'] < rg
    for i in range(c['G']):
        assert torch.equal(c['y'][i * rg + c['dom']], P.DOMINANT * c['y'][i * rg + c['dom'] - 1])
    assert float(c['gamma'].abs().min()) >= 0.25 and (C == 1 or (bool((c['gamma'] > 0).any()) and bool((c['gamma'] < 0).any())))
    assert not torch.equal(c['mean'], torch.zeros(C)) and not torch.equal(c['var'], torch.ones(C))
    gout, share = P.rows_probe(name)
    assert share <= P.MAX_ZEROED, (name, share)                   # a condition on the seed, not a measurement
    r64, r32 = P.rows_reference(name, 'float64'), P.rows_reference(name, 'float32')
    live = gout != 0
    if c['slope'] != 1.0:                                         # slope 1 has no kink
        assert torch.equal(r64['pre'][live] > 0, r32['pre'][live] > 0)
    for t in P.rows_compared(name):
        assert P.err(r32[t], r64[t]) < 1e-4, (name, t)


@pytest.mark.parametrize('name', POOL)
def test_pool_inputs_and_probe(name):
    c = P.pool_inputs(name)
    B, N, C, G = c['B'], c['N'], c['C'], c['G']
    assert c['zeroed'] <= P.MAX_ZEROED, (name, c['zeroed'])       # a condition on the seed, not a measurement
    assert float(c['gamma'].abs().min()) >= 0.25 and bool((c['gamma'] > 0).any()) and bool((c['gamma'] < 0).any())
    r64, r32 = P.pool_reference(name, 'float64'), P.pool_reference(name, 'float32')
    assert torch.equal(r64['nstar'], c['nstar'])
    live = c['gout'][:, :C] != 0
    assert torch.equal(r64['nstar'][live], r32['nstar'][live])     # the fp32 form's own choice
    assert torch.equal(r64['pre'] > 0, r32['pre'] > 0)             # no pre-activation within KINK1 of the kink: every row
    for t in P.pool_compared(name):
        assert P.err(r32[t], r64[t]) < 1e-4, (name, t)


@pytest.mark.parametrize('kind', ['chunk', 'lane', 'first'])
def test_tie_cases_route_to_the_first_of_the_two_rows(kind):
    name = 'tie-' + kind
    c = P.pool_inputs(name)
    n1, n2 = P.TIE_ROWS[kind]
    Bg = c['B'] // c['G']
    for g in range(c['G']):
        b = g * Bg                                                # cloud 0 of the group
        assert torch.equal(c['y'][b, n2], c['y'][b, n1]) and torch.equal(c['y'][b, n1], P.DOMINANT * c['y'][b, n1 - 1])
        ns = c['nstar'][b]
        assert not bool((ns == n2).any())
        won = ns == n1
        assert float(won.double().mean()) >= 0.2 and bool(won[c['gamma'] > 0].any()) and bool(won[c['gamma'] < 0].any()), (name, g)
        assert bool((c['gout'][b, :c['C']][won] != 0).all())       # copies of the winner do not count as a small gap


def test_constant_channels_route_to_row_0():
    c = P.pool_inputs('tie-const')
    Bg = c['B'] // c['G']
    assert float(c['gamma'][0]) > 0 > float(c['gamma'][1])
    r = P.pool_reference('tie-const', 'float64')
    for g in range(c['G']):
        b = g * Bg
        assert bool((c['y'][b, :, :2] == 0.5).all()) and not bool((c['y'][b + 1, :, :2] == 0.5).any())
        assert c['nstar'][b, :2].tolist() == [0, 0] and bool((c['gout'][b, :2] != 0).all())
        a = P.act(r['pre'][b, :, :2], c['slope'])
        assert bool((a == a[0]).all())


# ----------------------------------------------------------------------------- the restatements against the composed forms
def _grads(out, leaves, probe):
    return torch.autograd.grad(out, leaves, probe)


@pytest.mark.parametrize('name', ROWS)
def test_rows_restatement_is_batch_norm_and_leaky_relu(name):
    c = P.rows_inputs(name)
    r = P.rows_reference(name, 'float64')
    leaves = [t.double().clone().requires_grad_(True) for t in (c['y'], c['gamma'], c['beta'])]
    out, rm, rv = P.naive_rows(c, *leaves)
    assert P.err(out, r['out']) < 1e-12 and P.err(rm, r['mean']) < 1e-12 and P.err(rv, r['var']) < 1e-12
    for got, t in zip(_grads(out, leaves, P.rows_probe(name)[0].double()), ('dy', 'dgamma', 'dbeta')):
        assert P.err(got, r[t]) < 1e-9, (name, t)
    if c['train']:                                                # the buffers are the recurrence over the groups' own moments
        m, _, u = P.moments(c['y'].double(), c['G'])
        rm2, rv2 = P.recurrence(c['mean'].double(), c['var'].double(), m, u)
        assert P.err(rm2, r['mean']) < 1e-12 and P.err(rv2, r['var']) < 1e-12
    else:
        assert torch.equal(r['mean'], c['mean'].double()) and torch.equal(r['var'], c['var'].double())


@pytest.mark.parametrize('name', TIE_FREE_POOL)
def test_pool_restatement_is_batch_norm_leaky_relu_max_and_mean(name):
    c = P.pool_inputs(name)
    r = P.pool_reference(name, 'float64')
    leaves = [t.double().clone().requires_grad_(True) for t in (c['y'], c['gamma'], c['beta'])]
    out, rm, rv = P.naive_pool(c, *leaves)
    assert P.err(out, r['out']) < 1e-12 and P.err(rm, r['mean']) < 1e-12 and P.err(rv, r['var']) < 1e-12
    for got, t in zip(_grads(out, leaves, c['gout'].double()), ('dy', 'dgamma', 'dbeta')):
        assert P.err(got, r[t]) < 1e-9, (name, t)


@pytest.mark.parametrize('name', STATS)
def test_stats_inputs(name):
    c = P.stats_inputs(name)
    rg = c['rows'] // c['G']
    for i in range(c['G']):
        assert torch.equal(c['y'][i * rg + P.DOM_ROW], P.DOMINANT * c['y'][i * rg + P.DOM_ROW - 1])
    k64, k32 = P.coef_rows(c, c['y'], torch.float64), P.coef_rows(c, c['y'], torch.float32)
    assert tuple(k64.shape) == (c['G'], 5, c['C']) and P.err(k32, k64) < 1e-4
    # rows 0 and 1 are the affine form of BatchNorm with the group's moments
    want = torch.nn.functional.batch_norm(c['y'][:rg].double(), None, None, c['gamma'].double(), c['beta'].double(), True, 0.0, P.EPS)
    assert P.err(c['y'][:rg].double() * k64[0, 0] + k64[0, 1], want) < 1e-12
