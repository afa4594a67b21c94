"""CPU: the fp64 restatements of tests/pointmlp_cases.py are right, and its cases are what tests/test_gpu_pointmlp_fp64.py
relies on: exact products and ties on the grid, few zeroed probes, the planted rows, every dispatch path of the table."""
import pytest
import torch
import torch.nn.functional as F

import pointmlp_cases as C

ALL = C.case_list()
IDS = ['%s-%s%s' % (c, f, '-shift' if s else '') for c, f, s in ALL]


def _tiny(G, seed=0):
    g = C.gen('tiny', G, seed)
    S, seg, K, Co = 4, 4, 3, 5
    t = {'x': torch.randn(S * seg, K, generator=g), 'W': torch.randn(Co, K, generator=g), 'b': torch.randn(Co, generator=g),
         'gamma': torch.tensor([1.3, -0.7, 0.0, 0.9, -1.1]), 'beta': torch.tensor([0.3, -0.4, 0.5, -0.6, 0.7]),
         'g1': torch.tensor([0.8, -1.2, 1.1]), 'be1': torch.tensor([0.35, -0.45, 0.25])}
    t = {k: v.double() for k, v in t.items()}
    t['n'] = torch.randint(0, seg, (S, Co), generator=g)
    t['rm'], t['rv'] = torch.linspace(-0.2, 0.2, Co).double(), torch.linspace(0.5, 1.5, Co).double()
    t['rm1'], t['rv1'] = torch.linspace(-0.1, 0.1, K).double(), torch.linspace(0.7, 1.2, K).double()
    return t, seg


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('G', [1, 2])
def test_gradcheck_of_the_fp64_restatements_with_a_fixed_routing(G, train):
    """Both restatements against numeric derivatives; n* is held fixed so that the numeric derivative sees no jumps."""
    t, seg = _tiny(G)
    leaves = [t[k].clone().requires_grad_(True) for k in ('x', 'W', 'b', 'gamma', 'beta')]

    def plain(x, W, b, gamma, beta):
        out, pre, _, _ = C.layer(x, W, b, gamma, beta, t['rm'], t['rv'], 0.2, seg, G, train, t['n'])
        assert float(pre.detach().abs().min()) > 1e-3                   # off the kink of the activation
        return out

    assert torch.autograd.gradcheck(plain, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)
    leaves = [t[k].clone().requires_grad_(True) for k in ('x', 'g1', 'be1', 'W', 'b', 'gamma', 'beta')]

    def xf(y, g1, be1, W, b, gamma, beta):
        pre1 = C._bn(y, g1, be1, t['rm1'], t['rv1'], G, train)[0]
        assert float(pre1.detach().abs().min()) > 1e-3
        z = C._act(pre1, 0.1)
        return C.layer(z, W, b, gamma, beta, t['rm'], t['rv'], 0.2, seg, G, train, t['n'])[0], z

    assert torch.autograd.gradcheck(xf, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)
    # the public restatements return exactly these functions' gradients
    po, pz = torch.randn(4, 5, generator=C.gen('po')).double(), torch.randn(16, 3, generator=C.gen('pz')).double()
    r = C.pointmlp_max_ref(t['x'], t['W'], t['b'], t['gamma'], t['beta'], (t['rm'], t['rv']), 0.2, seg, G, train, torch.float64,
                           probe=po, nstar=t['n'])
    want = torch.autograd.grad(plain(*leaves[:1], *leaves[3:]), [leaves[0]] + leaves[3:], po)
    for k, w in zip(('dx', 'dW', 'db', 'dgamma', 'dbeta'), want):
        assert torch.equal(r[k], w), k
    r = C.bn_act_pointmlp_max_ref(t['x'], t['g1'], t['be1'], (t['rm1'], t['rv1']), 0.1, t['W'], t['b'], t['gamma'], t['beta'],
                                  (t['rm'], t['rv']), 0.2, seg, G, train, torch.float64, probe=po, probe_z=pz, nstar=t['n'])
    want = torch.autograd.grad(xf(*leaves), leaves, [po, pz])
    for k, w in zip(('dy', 'dgamma1', 'dbeta1', 'dW', 'db', 'dgamma', 'dbeta'), want):
        assert torch.equal(r[k], w), k


def test_xf_restatement_returns_none_where_no_gradient_flows():
    t, seg = _tiny(1)
    pz = torch.randn(16, 3, generator=C.gen('pz')).double()
    args = (t['x'], t['g1'], t['be1'], (t['rm1'], t['rv1']), 0.1, t['W'], t['b'], t['gamma'], t['beta'], (t['rm'], t['rv']), 0.2,
            seg, 1, True, torch.float64)
    r = C.bn_act_pointmlp_max_ref(*args, probe=None, probe_z=pz)
    assert all(r[k] is None for k in ('dW', 'db', 'dgamma', 'dbeta')) and all(r[k] is not None for k in ('dy', 'dgamma1', 'dbeta1'))
    r = C.bn_act_pointmlp_max_ref(*args, probe=torch.ones(4, 5).double(), wrt=('W', 'gamma'))
    assert sorted(k for k in r if k.startswith('d')) == ['dW', 'dgamma']


@pytest.mark.parametrize('case', ['groups', 'seg64a', 'seg64b', 'seg96', 'split384'])
def test_fp64_restatement_equals_the_torch_composition(case):
    """F.linear + F.batch_norm + leaky_relu + segment max in fp64: the same values (a maximum does not depend on which of
    the tied rows is named), the same running buffers, and the same row wherever there is no tie."""
    c = C.build(case, 'gauss')
    r = C.reference(case, 'gauss', 0.0, 'float64')
    rm, rv = c['mean'].double().clone(), c['var'].double().clone()
    outs, args = [], []
    for xg in c['x'].double().chunk(c['G']):
        y = F.linear(xg, c['W'].double(), None if c['b'] is None else c['b'].double())
        z = F.leaky_relu(F.batch_norm(y, rm, rv, c['gamma'].double(), c['beta'].double(), c['train'], C.MOMENTUM, C.EPS), c['slope'])
        z = z.view(-1, c['seg'], c['Co'])
        outs.append(z.max(dim=1).values)
        args.append(torch.where(c['gamma'] >= 0, y, -y).view(-1, c['seg'], c['Co']).argmax(dim=1))
    torch.testing.assert_close(r['out'], torch.cat(outs), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r['mean'], rm, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r['var'], rv, rtol=1e-12, atol=1e-13)
    p1 = C.planted(c['S'], c['seg'], c['G'])[0]
    untied = (r['gap'] > 0) & (r['nstar'] != p1[:, None])              # (the winner p1 is tied with its copy by construction)
    assert float(untied.double().mean()) > 0.4
    assert torch.equal(r['nstar'][untied], torch.cat(args)[untied])


@pytest.mark.parametrize('case,family,shift', [t for t in ALL if t[1] == 'grid'], ids=[i for i, t in zip(IDS, ALL) if t[1] == 'grid'])
def test_grid_cases_are_exact_in_fp32_and_tied(case, family, shift):
    c = C.build(case, family, shift)
    y32 = c['x'] @ c['W'].t()
    y64 = c['x'].double() @ c['W'].double().t()
    if c['b'] is not None:
        y32, y64 = y32 + c['b'], y64 + c['b'].double()
    assert torch.equal(y32.double(), y64)
    # and in any summation order: every term is a multiple of 1/4 and the sum of magnitudes stays far below 2^24 / 4
    assert float(c['x'].abs().max()) * c['K'] + 1 < 2 ** 20 and bool((c['x'] * 2 == (c['x'] * 2).round()).all())
    r64, r32 = C.reference(case, family, shift, 'float64'), C.reference(case, family, shift, 'float32')
    assert torch.equal(r64['nstar'], r32['nstar']) and torch.equal(r64['zext'], r32['zext'].double())
    f = torch.where(c['gamma'] >= 0, y64, -y64).view(c['S'], c['seg'], c['Co'])
    at_extreme = (f == f.max(dim=1, keepdim=True).values).sum(dim=1)
    tied, natural = float((at_extreme > 1).double().mean()), float((r64['gap'] == 0).double().mean())
    print('pointmlp-ties %s%s rows tied at the extreme %.4f, of different values of x %.4f' % (case, '-shift' if shift else '', tied, natural))
    assert tied >= 0.03
    assert natural >= 0.01                      # ties that are no planted copies: 2 - 7 % of the pairs


@pytest.mark.parametrize('case,family,shift', ALL, ids=IDS)
def test_zeroed_probe_share_and_planted_rows(case, family, shift):
    c = C.build(case, family, shift)
    r = C.reference(case, family, shift, 'float64')
    _planted_and_zeroed(c, r, c['x'])


@pytest.mark.parametrize('case', list(C.XF_CASES))
def test_xf_cases_zeroed_probe_share_and_planted_rows(case):
    c = C.build_xf(case)
    r = C.reference_xf(case, 'float64', 'plain')
    _planted_and_zeroed(c, r, c['y'])
    pre1 = C._bn(c['y'].double(), c['gamma1'].double(), c['beta1'].double(), c['mean1'].double(), c['var1'].double(), c['G'], c['train'])[0]
    assert float(pre1.abs().min()) >= 1e-3


def _planted_and_zeroed(c, r, x):
    S, seg = c['S'], c['seg']
    assert c['zeroed'] <= 0.01 and float((c['gout'] == 0).double().mean()) == c['zeroed']
    assert c['family'] == 'gauss' or c['zeroed'] <= 0.005          # the grid: the kink of the activation only
    p1, p2, q = C.planted(S, seg, c['G'])
    s0 = torch.arange(S) * seg
    assert bool((p2 > p1).all()) and torch.equal(x[s0 + p1], x[s0 + p2])
    if seg > 32:
        assert bool((p2 // 32 != p1 // 32).all())
    if seg >= 1024:
        assert bool((p2 // (seg // 8) != p1 // (seg // 8)).all())               # another part of a segment split 8 ways
    if S >= 5:
        assert {0, 31}.issubset(set(p1.tolist()) | set(p2.tolist())) and seg - 1 in p2.tolist()
        assert seg == 32 or 32 in (set(p1.tolist()) | set(p2.tolist()))
    n = r['nstar']
    share = (n == p1[:, None]).double().mean(dim=1)
    assert float(share.min()) >= 0.25, share.min()
    assert int((n == p2[:, None]).sum()) == 0
    assert int((share * c['Co']).min()) >= 24                 # dozens of channels of a segment pick the same row


def test_positions_over_all_cases_include_0_31_32_and_the_last_row():
    seen, most = {}, {}
    for case, spec in list(C.CASES.items()) + list(C.XF_CASES.items()):
        p1, p2, _ = C.planted(spec['S'], spec['seg'], spec['G'])
        seen.setdefault(spec['seg'], set()).update(p1.tolist() + p2.tolist())
        most[spec['seg']] = max(most.get(spec['seg'], 0), spec['S'])
    for seg, pos in seen.items():
        assert {0, 31, seg - 1}.issubset(pos), seg
        assert seg == 32 or most[seg] < 3 or 32 in pos, seg            # (two segments of 2048 rows hold two patterns)


def test_paths_cover_every_instantiation_and_branch_of_the_table():
    tags = set()
    for case in list(C.CASES) + list(C.XF_CASES):
        tags |= C.paths(case, 256)['tags']
    missing = [t for t in C.REQUIRED_TAGS if t not in tags]
    assert not missing, missing
    p = {case: C.paths(case, 256) for case in list(C.CASES) + list(C.XF_CASES)}
    assert [p['tiles%d' % i]['tiles'] for i in range(1, 6)] == [1, 2, 3, 4, 5]
    assert (p['partial']['nrb'], p['partial']['last_tiles']) == (2, 8) and p['partial']['dx'] == 'dx_seg<2,2>'
    assert p['seg64a']['dx'] == 'dx_seg<1,4>' and p['seg64b']['dx'] == 'dx_seg<2,4>' and p['tiles3']['dx'] == 'dx_seg<1,2>'
    assert (p['seg96']['dx'], p['seg96']['chunks'], p['seg96']['tiles']) == ('dx<1>:small-Co', 4, 18)
    assert p['seg128']['dx'] == 'dx<2>:small-Co'
    assert (p['split']['parts'], p['split']['nrb'], p['split']['dx']) == (8, 16, 'dx<2>:large-Co')
    assert (p['split384']['parts'], p['split384']['nrb'], p['split384']['dx']) == (8, 16, 'dx<1>:large-Co')
    assert (p['seg2048']['parts'], p['seg2048']['rpw']) == (8, 256)
    assert (p['xcd']['parts'], p['xcd']['nrb']) == (1, 8)
    assert (p['whole1024']['parts'], p['whole1024']['nrb'], p['whole1024']['dx']) == (1, 128, 'dx<1>:large-Co')
    assert p['xf_split']['parts'] == 8
    # the grid-stride shapes: a second trip of the general and of the per-wave kernel
    s = {k: C.bwd_paths(v['S'], v['seg'], v['K'], v['Co'], 256) for k, v in C.SPARSE_CASES.items()}
    assert (s['general-trips']['dx'], s['general-trips']['trips']) == ('dx<1>:large-Co', 2)
    assert (s['per-wave-trips']['dx'], s['per-wave-trips']['trips']) == ('dx_seg<1,2>', 2)
    # fewer compute units only ever split less
    assert C.paths('split', 64)['parts'] == 8 and C.paths('split', 8)['parts'] < 8


@pytest.mark.parametrize('case,family,shift', [('tiles3', 'gauss', 0.0), ('seg128', 'gauss', 0.0), ('split', 'grid', 8.0), ('seg64b', 'grid', 0.0)])
def test_fp32_restatement_is_close_to_fp64_but_not_equal(case, family, shift):
    r64, r32 = C.reference(case, family, shift, 'float64'), C.reference(case, family, shift, 'float32')
    train = C.CASES[case]['train']
    for k in ('out', 'dx', 'dW', 'dgamma', 'dbeta') + (('mean', 'var') if train else ('db',)):
        e = C.err(r32[k], r64[k])
        assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64
        assert 0.0 < e < 2e-5, (k, e)
    for option in ('grad_at_z', 'z_only'):
        x64, x32 = C.reference_xf('xf_sa1', 'float64', option), C.reference_xf('xf_sa1', 'float32', option)
        for k in ('out', 'z', 'dy', 'dgamma1', 'dbeta1'):
            assert 0.0 < C.err(x32[k], x64[k]) < 2e-5, (option, k)
