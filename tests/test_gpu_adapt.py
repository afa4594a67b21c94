"""GPU: the SA-node glue kernels of sug_amd/csrc/adapt.hip (node_offset, interp3_cat) on every dispatch path against the
fp64 restatements of tests/adapt_cases.py.

Bound, per output tensor (adapt_cases.err / within):  err(x) = max|x - ref64| / max(max|ref64|, tiny)  and
err(kernel) <= 8 * err(the same formula in plain fp32 torch, same inputs) + 1e-7.  Every element of every output is
compared.  Each test prints `adapt-ratio <group> <case> <tensor> err(kernel) err(fp32 torch)` before it asserts.

Every outcome of sug_node_offset_bwd's dispatcher is named in a test id: P8 / P4 / P2 / P1 (ordered kernel, accumulator
planes), global-atomic (N > 9600), and lds-atomic / global-atomic under SUG_NODE_OFFSET_UNORDERED=1 (child process).
The two backward forms of interp3_cat are `lists` (sorted reverse lists, the default) and `lds` (LDS accumulation + float
atomics: sug_interp3_cat_bwd, the fall-back beyond the list-resident size)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import adapt_cases as C
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _path(N):
    """The outcome of sug_node_offset_bwd's dispatcher for N points per cloud (16 N P <= 150 KB)."""
    return 'P8' if N <= 1200 else 'P4' if N <= 2400 else 'P2' if N <= 4800 else 'P1' if N <= 9600 else 'global-atomic'


def _bound(group, case, errs):
    for k, (ek, e32) in errs.items():
        print('adapt-ratio %s %s %s %.4g %.4g' % (group, case, k, ek, e32))
    bad = {k: v for k, v in errs.items() if not C.within(*v)}
    assert not bad, '%s %s: err(kernel), err(fp32 torch) = %r' % (group, case, bad)


def _node_offset(group, pattern, N, S, ns, B=2):
    c = C.node_case(pattern, B, N, S, ns)
    got, errs = C.measure_node_offset(c)
    _bound(group, '%s-N%d-S%d-ns%d-%s' % (_path(N), N, S, ns, pattern), errs)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    return c, got


def _sentinel_properties(c, got):
    un, em = ~C.named_points(c), C.empty_nodes(c)
    assert bool(un.any()) and bool(em.any())
    for k in ('off', 'nloc', 'both'):
        assert float(got['dproj/' + k][un].abs().max()) == 0.0, 'rows nobody names must be exactly 0 (%s)' % k
    N = c['proj'].shape[1]
    centre = C.rows(c['loc'], c['fidx'].long().clamp(0, N - 1))
    assert float(got['off'][em].abs().max()) == 0.0 and torch.equal(got['nloc'][em], centre[em])


# ----------------------------------------------------------------------------- node_offset
@pytest.mark.parametrize('N', [1200, 1201, 2400, 2401, 4800, 4801, 9600, 9601], ids=lambda N: '%s-N%d' % (_path(N), N))
def test_node_offset_dispatch_boundaries(N):
    _node_offset('node_offset/dispatch', 'padded', N, 64, 64)


@pytest.mark.parametrize('N,S', [pytest.param(N, S, id='%s-N%d-S%d' % (_path(N), N, S))
                                 for N, Ss in ((256, (1, 7, 8, 9, 15, 16, 17, 23)), (2048, (3, 5, 9))) for S in Ss])
def test_node_offset_pipeline_guards(N, S):
    """S < P, S = P + 1, S no multiple of P: the guards of the two-deep load pipeline of the ns <= 64 branch."""
    for pattern in ('random', 'padded'):
        _node_offset('node_offset/pipeline', pattern, N, S, 64)


@pytest.mark.parametrize('pattern', ['few', 'constant', 'sentinel'])
@pytest.mark.parametrize('ns', [1, 16, 63, 64, 65, 128, 130], ids=lambda ns: 'P8-ns%d' % ns)
def test_node_offset_list_lengths(ns, pattern):
    """Both branches (ns <= 64 pipelined, ns > 64 trips of 64), lane padding, duplicates across trips, a centre that is
    its own neighbour."""
    c, got = _node_offset('node_offset/ns', pattern, 256, 10, ns)
    if pattern == 'sentinel':
        _sentinel_properties(c, got)


@pytest.mark.parametrize('N', [256, 2048, 4096, 8192, 9601], ids=lambda N: '%s-N%d' % (_path(N), N))
def test_node_offset_sentinels(N):
    """n == N (a zero-hit ball-query row), n < 0 and centres outside [0, N): three differently written guards."""
    c, got = _node_offset('node_offset/sentinel', 'sentinel', N, 64, 64)
    _sentinel_properties(c, got)


@pytest.mark.parametrize('N', [1024, 2048, 4096, 8192], ids=lambda N: '%s-N%d' % (_path(N), N))
def test_node_offset_backward_reproducible(N):
    """The ordered kernel at every plane count: three backward calls are bit-identical on the worst collisions."""
    c = C.node_case('few', 2, N, 64, 64)
    runs = [C.run_node_offset(c) for _ in range(3)]
    for k in ('dproj/off', 'dproj/nloc', 'dproj/both'):
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k
    _bound('node_offset/reproducible', '%s-N%d-few' % (_path(N), N),
           C.errors(runs[0], C.node_offset_all(c, torch.float64), C.node_offset_all(c, torch.float32)))


def test_node_offset_unordered_lds_atomic_and_global_atomic(tmp_path):
    """SUG_NODE_OFFSET_UNORDERED=1 (read once per process: one child for all cases): the LDS-atomic kernel at N = 1024
    and the global-atomic kernel at N = 6000, same bound."""
    out = str(tmp_path / 'unordered.json')
    env = dict(os.environ, SUG_NODE_OFFSET_UNORDERED='1')
    r = subprocess.run([sys.executable, 'tests/adapt_cases.py', '--unordered', out], env=env, cwd=ROOT, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    assert sorted(res) == sorted('%s-N%d-%s' % t for t in C.UNORDERED_CASES)
    for case, v in res.items():
        _bound('node_offset/unordered', case, {k: tuple(e) for k, e in v['errors'].items()})
        assert v['empty_max'] == 0.0, case
        if 'sentinel' in case:
            assert v['unnamed_max'] == 0.0, case


# ----------------------------------------------------------------------------- interp3_cat
def _vp(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _interp_ops(c):
    """Through ops.interp3_cat -> (outputs, idx3, d3): d3 and idx3 read back with the 3-NN the op itself runs."""
    from sug_amd import ops
    fea, node, nloc = (c[k].cuda().requires_grad_(True) for k in ('fea', 'node', 'nloc'))
    xyz = c['xyz'].cuda()
    out = ops.interp3_cat(fea, node, xyz, nloc)
    dfea, dnode, dnloc = torch.autograd.grad(out, (fea, node, nloc), c['g'].cuda())
    idx3, d3 = ops.three_nn_raw(xyz, nloc.detach())
    return {'out': out.detach(), 'dfea': dfea, 'dnode': dnode, 'dnloc': dnloc}, idx3, d3


def _interp_direct(c, idx3, d3, form, pad_f=0, pad_go=0):
    """sug_interp3_cat_fwd and one backward entry point called directly: fea a column slice (from column 4) of a buffer
    pad_f wider than C1, out and g rows pad_go wider than C1 + C2 -> {'out', 'dnode', 'dnloc'}."""
    from sug_amd._lib import lib, check
    L = lib()
    B, N, C1 = c['fea'].shape
    S, C2 = c['node'].shape[1:]
    wide = torch.full((B, N, C1 + pad_f), 3.0, device='cuda')
    off = 4 if pad_f else 0
    wide[:, :, off:off + C1] = c['fea'].cuda()
    node, xyz, nloc = c['node'].cuda(), c['xyz'].cuda(), c['nloc'].cuda()
    ld = C1 + C2 + pad_go
    out = torch.full((B, N, ld), 7.0, device='cuda')
    g = torch.full((B, N, ld), 5.0, device='cuda')
    g[:, :, :C1 + C2] = c['g'].cuda()
    check(L.sug_interp3_cat_fwd(_vp(wide, 4 * off) if C1 else None, (C1 + pad_f) if C1 else 0, C1, _vp(node), _vp(idx3), _vp(d3),
                                B, N, S, C2, _vp(out), ld, _stream()), 'sug_interp3_cat_fwd')
    if form == 'lists':
        dnode, dnloc = torch.full((B, S, C2), 9.0, device='cuda'), torch.full((B, S, 3), 9.0, device='cuda')   # written entirely
        roff = torch.empty(B, S + 1, dtype=torch.int32, device='cuda')
        rent = torch.empty(B, 3 * N, dtype=torch.int32, device='cuda')
        ddw = torch.empty(B, N, 6, device='cuda')
        check(L.sug_interp3_cat_bwd_lists(_vp(g), ld, C1, _vp(node), _vp(idx3), _vp(d3), _vp(xyz), _vp(nloc), B, N, S, C2,
                                          _vp(roff), _vp(rent), _vp(ddw), _vp(dnode), _vp(dnloc), _stream()),
              'sug_interp3_cat_bwd_lists')
    else:
        dnode, dnloc = torch.zeros(B, S, C2, device='cuda'), torch.zeros(B, S, 3, device='cuda')
        check(L.sug_interp3_cat_bwd(_vp(g), ld, C1, _vp(node), _vp(idx3), _vp(d3), _vp(xyz), _vp(nloc), B, N, S, C2,
                                    _vp(dnode), _vp(dnloc), _stream()), 'sug_interp3_cat_bwd')
    torch.cuda.synchronize()
    assert bool((out[:, :, C1 + C2:] == 7.0).all()), 'the forward wrote outside its C1 + C2 columns'
    return {'out': out[:, :, :C1 + C2], 'dnode': dnode, 'dnloc': dnloc}


def _interp_bound(group, case, c, got, idx3, d3):
    r64, r32 = C.interp3_cat_all(c, idx3, d3, torch.float64), C.interp3_cat_all(c, idx3, d3, torch.float32)
    _bound(group, case, C.errors(got, r64, r32))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    return r64


def _unused_nodes(idx3, B, S):
    used = torch.zeros(B, S, dtype=torch.bool)
    used.scatter_(1, idx3.cpu().long().reshape(B, -1), True)
    return ~used


@pytest.mark.parametrize('C1,C2', [pytest.param(*t, id='lists-C1_%d-C2_%d' % t)
                                   for t in ((64, 64), (0, 64), (4, 4), (68, 36), (64, 68), (64, 128), (128, 64))])
def test_interp3_cat_channels(C1, C2):
    c = C.interp_case(2, 300, 64, C1, C2)
    got, idx3, d3 = _interp_ops(c)
    _interp_bound('interp3_cat/channels', 'lists-C1_%d-C2_%d' % (C1, C2), c, got, idx3, d3)
    assert torch.equal(got['dfea'].cpu(), c['g'][:, :, :C1])


@pytest.mark.parametrize('variant', ['ldf', 'ldg-ldo', 'both'])
@pytest.mark.parametrize('form', ['lists', 'lds'])
def test_interp3_cat_strides(form, variant):
    """fea a column slice of a wider buffer (ldf = C1 + 8); out / g rows wider than C1 + C2."""
    from sug_amd import ops
    c = C.interp_case(2, 300, 64, 68, 36, 'strides')
    idx3, d3 = ops.three_nn_raw(c['xyz'].cuda(), c['nloc'].cuda())
    got = _interp_direct(c, idx3, d3, form, pad_f=8 if variant != 'ldg-ldo' else 0, pad_go=12 if variant != 'ldf' else 0)
    _interp_bound('interp3_cat/strides', '%s-%s' % (form, variant), c, got, idx3, d3)


@pytest.mark.parametrize('S,N', [pytest.param(*t, id='lists-S%d-N%d' % t)
                                 for t in ((3, 257), (4, 257), (64, 257), (200, 257), (200, 50))])
def test_interp3_cat_node_counts(S, N):
    """BN % 16 != 0 and BS % 16 != 0; the minimum S; nodes that no point interpolates from get exactly 0."""
    c = C.interp_case(2, N, S, 4, 68)
    got, idx3, d3 = _interp_ops(c)
    _interp_bound('interp3_cat/S', 'lists-S%d-N%d' % (S, N), c, got, idx3, d3)
    un = _unused_nodes(idx3, 2, S)
    if N == 50:
        assert int(un.sum()) >= 2 * (S - 3 * N)            # at most 150 of the 200 nodes of a cloud are named
    if un.any():
        assert float(got['dnode'].cpu()[un].abs().max()) == 0.0 and float(got['dnloc'].cpu()[un].abs().max()) == 0.0
    assert torch.equal(got['dfea'].cpu(), c['g'][:, :, :4])


@pytest.mark.parametrize('form', ['lists', 'lds'])
def test_interp3_cat_clamp(form):
    """d < 1e-10: the forward weight comes from 1/1e-10, the backward sends nothing through the clamped distance.
    Nodes 0..9 sit exactly on points (d3 == 0 with the direct-form 3-NN); nodes 10..19 sit 1e-6 beside a point
    (d3 ~ 1e-12: clamped, and 2 (nloc - xyz) != 0, so an unclamped term would show as a gradient of order 1e4)."""
    from sug_amd import ops
    B, N, S = 2, 300, 64
    c = C.interp_case(B, N, S, 4, 36, 'clamp')
    pts = torch.randperm(N, generator=C.gen('clamp-points'))[:20]
    c['nloc'][:, :20] = c['xyz'][:, pts]
    c['nloc'][:, 10:20, 0] += 1e-6
    idx3, d3 = ops.three_nn_raw(c['xyz'].cuda(), c['nloc'].cuda(), direct=True)
    d0, i0 = d3.cpu()[:, pts, 0], idx3.cpu()[:, pts, 0].long()
    assert bool((d0[:, :10] == 0).all()) and bool((d0[:, 10:] > 0).all()) and bool((d0[:, 10:] < 1e-10).all())
    assert torch.equal(i0, torch.arange(20).expand(B, 20))
    got = _interp_direct(c, idx3, d3, form)
    _interp_bound('interp3_cat/clamp', form, c, got, idx3, d3)
    # only the clamped points carry gradient: their own node (term 0, clamped) must receive exactly nothing
    probe = dict(c, g=torch.zeros_like(c['g']))
    probe['g'][:, pts] = c['g'][:, pts]
    named_twice = torch.zeros(B, S, dtype=torch.bool)
    named_twice.scatter_(1, idx3.cpu()[:, pts, 1:].long().reshape(B, -1), True)
    got = _interp_direct(probe, idx3, d3, form)
    _interp_bound('interp3_cat/clamp', form + '-probe', probe, got, idx3, d3)
    alone = ~named_twice
    alone[:, 20:] = False
    assert bool(alone.any())
    assert float(got['dnloc'].cpu()[alone].abs().max()) == 0.0
    assert float(got['dnloc'].cpu()[named_twice].abs().max()) > 0.0


@pytest.mark.parametrize('C1,C2,S,N', [pytest.param(*t, id='lds-C1_%d-C2_%d-S%d-N%d' % t)
                                       for t in ((64, 64, 64, 1000), (4, 36, 3, 65), (64, 128, 100, 300))])
def test_interp3_cat_legacy_lds_form(C1, C2, S, N):
    """sug_interp3_cat_bwd (LDS accumulation, float atomics into zero-filled gradients) under the same bound."""
    from sug_amd import ops
    c = C.interp_case(2, N, S, C1, C2, 'legacy')
    idx3, d3 = ops.three_nn_raw(c['xyz'].cuda(), c['nloc'].cuda())
    got = _interp_direct(c, idx3, d3, 'lds')
    _interp_bound('interp3_cat/lds', 'lds-C1_%d-C2_%d-S%d-N%d' % (C1, C2, S, N), c, got, idx3, d3)


def test_interp3_cat_legacy_lds_form_refuses_what_does_not_fit():
    """(S C2 + 3 S) * 4 > 64 KB: an error code with a message, no launch."""
    from sug_amd._lib import lib, check
    B, N, S, C2 = 2, 64, 256, 64
    shapes = {'g': (B, N, C2), 'node': (B, S, C2), 'd3': (B, N, 3), 'xyz': (B, N, 3), 'nloc': (B, S, 3), 'dnode': (B, S, C2),
              'dnloc': (B, S, 3)}
    t = {k: torch.zeros(s, device='cuda') for k, s in shapes.items()}
    idx3 = torch.zeros(B, N, 3, dtype=torch.int32, device='cuda')
    rc = lib().sug_interp3_cat_bwd(_vp(t['g']), C2, 0, _vp(t['node']), _vp(idx3), _vp(t['d3']), _vp(t['xyz']), _vp(t['nloc']),
                                   B, N, S, C2, _vp(t['dnode']), _vp(t['dnloc']), _stream())
    assert rc != 0
    with pytest.raises(RuntimeError, match='too large for the LDS accumulator'):
        check(rc, 'sug_interp3_cat_bwd')


def test_interp3_cat_large_n_falls_back_to_lds_form():
    """3 N entries per cloud beyond the LDS-resident reverse-list build: ops.interp3_cat's backward takes the
    LDS-accumulating form instead of raising (id: lds-fallback-N16384)."""
    from sug_amd._lib import lib
    B, N, S = 2, 16384, 8
    assert lib().sug_interp3_cat_bwd_lists_supported(B, N, S) == 0
    c = C.interp_case(B, N, S, 4, 8)
    got, idx3, d3 = _interp_ops(c)
    _interp_bound('interp3_cat/large-N', 'lds-fallback-N%d' % N, c, got, idx3, d3)
    assert torch.equal(got['dfea'].cpu(), c['g'][:, :, :4])


def test_interp3_cat_list_resident_large_n_reproducible():
    """N = 12288 still fits the reverse lists (id: lists-N12288): bit-identical over three calls, same bound."""
    from sug_amd._lib import lib
    B, N, S = 2, 12288, 8
    assert lib().sug_interp3_cat_bwd_lists_supported(B, N, S) == 1
    c = C.interp_case(B, N, S, 4, 8)
    runs = [_interp_ops(c) for _ in range(3)]
    for k in ('out', 'dfea', 'dnode', 'dnloc'):
        assert torch.equal(runs[0][0][k], runs[1][0][k]) and torch.equal(runs[0][0][k], runs[2][0][k]), k
    _interp_bound('interp3_cat/large-N', 'lists-N%d' % N, c, *runs[0])


# ----------------------------------------------------------------------------- argument guards
def _interp_args(entry, **over):
    """Valid arguments of one interp3_cat entry point at B=2, N=32, S=8, C1=4, C2=8, with overrides."""
    B, N, S, C1, C2 = (over.get(k, v) for k, v in (('B', 2), ('N', 32), ('S', 8), ('C1', 4), ('C2', 8)))
    z = lambda *s: torch.zeros(*[max(1, v) for v in s], device='cuda')
    t = {'fea': z(2, N, C1), 'node': z(2, S, C2 + 4), 'idx3': torch.zeros(2, N, 3, dtype=torch.int32, device='cuda'),
         'd3': torch.ones(2, N, 3, device='cuda'), 'out': z(2, N, C1 + C2), 'g': z(2, N, C1 + C2), 'xyz': z(2, N, 3),
         'nloc': z(2, S, 3), 'dnode': z(2, S, C2), 'dnloc': z(2, S, 3), 'ddw': z(2, N, 6),
         'roff': torch.zeros(2, S + 1, dtype=torch.int32, device='cuda'),
         'rent': torch.zeros(2, 3 * N, dtype=torch.int32, device='cuda')}
    p = {k: _vp(v) for k, v in t.items()}
    p.update({k: v for k, v in over.items() if k in p})
    if over.get('misaligned_node'):
        p['node'] = _vp(t['node'], 4)
    ld = C1 + C2
    if entry == 'fwd':
        args = (p['fea'], C1, C1, p['node'], p['idx3'], p['d3'], B, N, S, C2, p['out'], ld)
    elif entry == 'bwd':
        args = (p['g'], ld, C1, p['node'], p['idx3'], p['d3'], p['xyz'], p['nloc'], B, N, S, C2, p['dnode'], p['dnloc'])
    else:
        args = (p['g'], ld, C1, p['node'], p['idx3'], p['d3'], p['xyz'], p['nloc'], B, N, S, C2, p['roff'], p['rent'], p['ddw'],
                p['dnode'], p['dnloc'])
    return t, args + (_stream(),)


GUARDS = {'C2mod4': {'C2': 6}, 'S2': {'S': 2}, 'misaligned-node': {'misaligned_node': True}, 'null-node': {'node': None},
          'B0': {'B': 0}}


@pytest.mark.parametrize('guard', list(GUARDS))
@pytest.mark.parametrize('entry', ['fwd', 'bwd_lists', 'bwd'])
def test_interp3_cat_argument_guards(entry, guard):
    """SUG_REQUIRE: each of these comes back as a RuntimeError from check, not as a launch."""
    from sug_amd._lib import lib, check
    keep, ok = _interp_args(entry)
    check(getattr(lib(), 'sug_interp3_cat_' + entry)(*ok), entry)          # the unmodified arguments are accepted
    keep2, bad = _interp_args(entry, **GUARDS[guard])
    with pytest.raises(RuntimeError, match='null pointer' if guard == 'null-node' else 'bad shape|aligned'):
        check(getattr(lib(), 'sug_interp3_cat_' + entry)(*bad), entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize('guard', ['null-proj', 'null-gidx', 'B0', 'ns0'])
@pytest.mark.parametrize('entry', ['fwd', 'bwd'])
def test_node_offset_argument_guards(entry, guard):
    from sug_amd._lib import lib, check
    B, N, S, ns = 2, 32, 4, 8
    f = [torch.zeros(B, N, 3, device='cuda') for _ in range(2)]
    fidx = torch.zeros(B, S, dtype=torch.int32, device='cuda')
    gidx = torch.zeros(B, S, ns, dtype=torch.int32, device='cuda')
    o = [torch.zeros(B, S, 3, device='cuda') for _ in range(2)]
    dproj = torch.zeros(B, N, 3, device='cuda')
    proj = None if guard == 'null-proj' else _vp(f[0])
    gi = None if guard == 'null-gidx' else _vp(gidx)
    Bc, nsc = (0 if guard == 'B0' else B), (0 if guard == 'ns0' else ns)
    if entry == 'fwd':
        rc = lib().sug_node_offset_fwd(proj, _vp(f[1]), _vp(fidx), gi, Bc, N, S, nsc, _vp(o[0]), _vp(o[1]), _stream())
    else:
        rc = lib().sug_node_offset_bwd(proj, _vp(f[1]), _vp(fidx), gi, _vp(o[0]), Bc, N, S, nsc, _vp(dproj), _stream())
    with pytest.raises(RuntimeError, match='null pointer' if guard.startswith('null') else 'bad shape'):
        check(rc, entry)
    torch.cuda.synchronize()
