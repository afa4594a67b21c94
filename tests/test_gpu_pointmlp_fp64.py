"""GPU: the fused per-point MLP + max layer of sug_amd/csrc/pointmlp.hip (ops.pointmlp_max, ops.bn_act_pointmlp_max, and
sug_pointmlp_max_fwd / sug_pointmlp_max_bwd_sparse called directly) on every dispatch path against the fp64 restatements
of tests/pointmlp_cases.py.

Bound, per tensor and over every element (pointmlp_cases.err / within, the one of adapt_cases):
err(t) = max|t - ref64| / max(max|ref64|, tiny)  and  err(kernel) <= 8 * err(the same formula in plain fp32 torch) + 1e-7.
Each test prints `pointmlp-ratio <case> <family> <tensor> err(kernel) err(fp32 torch)` before it asserts.  On the grid
family the extreme and its row are compared exactly, ties included; on the gauss family the row is compared wherever the
fp64 gap is at least TAU_GAP * rms(y), and the probe is zero elsewhere, so every gradient is compared in every element.

Which path a case takes is `pointmlp_cases.paths(case, compute units of the device)`, printed as `pointmlp-path <case>
cus=<n> <tags>`; the raw-forward test holds the launcher's block count against it for every case.

Measured on an MI355X (256 compute units; all figures in profiles/pointmlp_fp64_ratios.txt): the worst ratio
err(kernel) / err(fp32 torch) per tensor is zext 1.0, out 1.8, running_mean 5.0 (seg96 gauss), running_var 2.4, dx 1.6,
dW 5.6 (split + 8, grid), dgamma 3.3, dbeta 1.6, db 1.3; XF: z 1.1, running_mean1 1.1, running_var1 0.7, dy 1.3,
dgamma1 1.3, dbeta1 3.5.  Every tensor holds the factor 8, so none has a factor of its own.  (With the dominant planted
row on the first row of a domain group, the pivot of the BatchNorm sums, the statistics did not: see pointmlp_cases.)"""
import ctypes

import pytest
import torch

import pointmlp_cases as C

pytestmark = pytest.mark.gpu

ALL = C.case_list()
IDS = ['%s-%s%s' % (c, f, '-shift' if s else '') for c, f, s in ALL]


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bound(case, family, got, r64, r32, keys=None):
    """Print err(kernel), err(fp32 torch) of every tensor of `got`, then assert the bound on each."""
    errs = {k: (C.err(got[k], r64[k]), C.err(r32[k], r64[k])) for k in (keys or got)}
    for k, (ek, e32) in errs.items():
        print('pointmlp-ratio %s %s %s %.4g %.4g' % (case, family, k, ek, e32))
    for k in errs:
        assert got[k].shape == r64[k].shape and bool(torch.isfinite(got[k]).all()), k
    bad = {k: v for k, v in errs.items() if not C.within(*v)}
    assert not bad, '%s %s: err(kernel), err(fp32 torch) = %r' % (case, family, bad)


def _bn_module(C_, gamma, beta, mean, var, train):
    bn = torch.nn.BatchNorm1d(C_, eps=C.EPS, momentum=C.MOMENTUM).cuda().train(train)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(mean), bn.running_var.copy_(var)
    assert torch.equal(torch.signbit(bn.weight.detach().cpu()), torch.signbit(gamma))           # -0.0 stays -0.0
    return bn


# ----------------------------------------------------------------------------- the forward kernel alone
@pytest.mark.parametrize('case,family,shift', ALL, ids=IDS)
def test_raw_forward_extreme_and_row(case, family, shift):
    """sug_pointmlp_max_fwd per domain group: arg == n* and zext == the extreme bit for bit on the grid; on gauss arg == n*
    wherever the gap is at least tau and zext within the bound everywhere.  The block count is that of paths()."""
    from sug_amd._lib import lib
    L = lib()
    c = C.build(case, family, shift)
    r64, r32 = C.reference(case, family, shift, 'float64'), C.reference(case, family, shift, 'float32')
    S, seg, K, Co, G = c['S'], c['seg'], c['K'], c['Co'], c['G']
    sg, rg = S // G, S * seg // G
    x, W, b, gam = c['x'].cuda(), c['W'].cuda(), None if c['b'] is None else c['b'].cuda(), c['gamma'].cuda()
    zext = torch.full((S, Co), float('nan'), device='cuda')
    arg = torch.full((S, Co), -1, dtype=torch.int32, device='cuda')
    p = C.paths(case, _cus())
    print('pointmlp-path %s cus=%d %s' % (case, _cus(), ' '.join(sorted(p['tags']))))
    for gi in range(G):
        ws = torch.zeros(1024 * 2 * Co, device='cuda')
        nblk = ctypes.c_int(0)
        xg = x[gi * rg:(gi + 1) * rg]
        rc = L.sug_pointmlp_max_fwd(_vp(xg), K, rg, K, _vp(W), _vp(b), _vp(gam), Co, seg, _vp(zext[gi * sg:(gi + 1) * sg]),
                                    _vp(arg[gi * sg:(gi + 1) * sg]), _vp(ws), ctypes.byref(nblk), _stream())
        assert rc == 0, L.sug_last_error()
        torch.cuda.synchronize()
        assert nblk.value == p['nrb'], 'row blocks %d, paths() %r' % (nblk.value, p)
        if p['parts'] > 1:
            assert nblk.value == sg * p['parts']
    if case in ('split', 'split384', 'seg2048') and _cus() == 256:
        assert p['parts'] == 8
    arg, zext = arg.cpu().long(), zext.cpu()
    assert int(arg.min()) >= 0 and int(arg.max()) < seg
    _bound(case, family, {'zext': zext}, r64, r32)
    if family == 'grid':
        assert torch.equal(arg, r64['nstar']), '%d rows differ' % int((arg != r64['nstar']).sum())
        assert torch.equal(zext.double(), r64['zext'])
    else:
        sure = r64['gap'] >= C.TAU_GAP * r64['rms']
        assert float(sure.double().mean()) >= 0.99
        assert torch.equal(arg[sure], r64['nstar'][sure]), '%d rows differ' % int((arg != r64['nstar'])[sure].sum())
    p2 = C.planted(S, seg, G)[1]
    assert int((arg == p2[:, None]).sum()) == 0                 # the later copy never wins


# ----------------------------------------------------------------------------- ops.pointmlp_max
class _DropGrad(torch.autograd.Function):
    """Identity whose backward hands back no gradient at all (None, not zeros)."""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return None


def _run_pointmlp_max(c, variant=None):
    from sug_amd import ops
    S, seg, K, Co, G = c['S'], c['seg'], c['K'], c['Co'], c['G']
    bn = _bn_module(Co, c['gamma'], c['beta'], c['mean'], c['var'], c['train'])
    n0 = int(bn.num_batches_tracked)
    W = c['W'].cuda().requires_grad_(True)
    b = None if c['b'] is None else c['b'].cuda().requires_grad_(True)
    if variant == 'xslice':                     # x a column slice of a wider buffer: row stride K + 8, no copy
        leaf = torch.full((S * seg, K + 8), 3.0, device='cuda')
        leaf[:, 4:4 + K] = c['x'].cuda()
        leaf.requires_grad_(True)
        x = leaf[:, 4:4 + K]
    else:
        leaf = x = c['x'].cuda().requires_grad_(True)
    with ops.bn_groups(G):
        out = ops.pointmlp_max(x, W, b, bn, c['slope'], seg)
        if variant == 'gslice':                 # the gradient a column slice of a wider one: the .contiguous() fall-back
            wide = torch.full((S, Co + 3), 5.0, device='cuda')
            wide[:, 3:] = c['gout'].cuda()
            out.backward(wide[:, 3:])
        elif variant == 'nograd':               # no gradient reaches out at all
            _DropGrad.apply(out).sum().backward()
        else:
            out.backward(c['gout'].cuda())
    torch.cuda.synchronize()
    dx = leaf.grad
    if variant == 'xslice':
        assert float(dx[:, :4].abs().max()) == 0.0 and float(dx[:, 4 + K:].abs().max()) == 0.0
        dx = dx[:, 4:4 + K]
    got = {'out': out.detach(), 'mean': bn.running_mean, 'var': bn.running_var, 'dx': dx, 'dW': W.grad,
           'dgamma': bn.weight.grad, 'dbeta': bn.bias.grad}
    if b is not None:
        got['db'] = b.grad
    assert int(bn.num_batches_tracked) == n0 + (G if c['train'] else 0)
    return {k: (None if v is None else v.detach().cpu()) for k, v in got.items()}


def _check_pointmlp_max(c, got, r64, r32, tag):
    keys = [k for k in got if k != 'db' or not c['train']]
    _bound(c['case'] + tag, c['family'], got, r64, r32, keys)
    if c['train'] and 'db' in got:
        assert float(got['db'].abs().max()) == 0.0              # a bias in front of train-mode BatchNorm: identically zero
    if not c['train']:
        assert torch.equal(got['mean'], c['mean']) and torch.equal(got['var'], c['var'])


@pytest.mark.parametrize('case,family,shift', ALL, ids=IDS)
def test_pointmlp_max_vs_fp64(case, family, shift):
    c = C.build(case, family, shift)
    got = _run_pointmlp_max(c)
    _check_pointmlp_max(c, got, C.reference(case, family, shift, 'float64'), C.reference(case, family, shift, 'float32'),
                        '-shift' if shift else '')


@pytest.mark.parametrize('variant', ['xslice', 'gslice', 'nograd'])
@pytest.mark.parametrize('case', ['seg64a', 'split'])
def test_pointmlp_max_strided_operands_and_no_gradient(case, variant):
    c = C.build(case, 'gauss')
    got = _run_pointmlp_max(c, variant)
    r64, r32 = C.reference(case, 'gauss', 0.0, 'float64'), C.reference(case, 'gauss', 0.0, 'float32')
    if variant != 'nograd':
        _check_pointmlp_max(c, got, r64, r32, '-' + variant)
        return
    _bound(case + '-nograd', 'gauss', got, r64, r32, ['out', 'mean', 'var'])
    for k in ('dx', 'dW', 'db', 'dgamma', 'dbeta'):             # an undefined gradient counts as zeros
        assert got[k] is None or float(got[k].abs().max()) == 0.0, k


# ----------------------------------------------------------------------------- ops.bn_act_pointmlp_max
@pytest.mark.parametrize('option', list(C.XF_OPTIONS))
@pytest.mark.parametrize('case', list(C.XF_CASES))
def test_bn_act_pointmlp_max_vs_fp64(case, option):
    from sug_amd import ops
    want_z, at_out, at_z, last_grad, wrt = C.XF_OPTIONS[option]
    c = C.build_xf(case)
    print('pointmlp-path %s cus=%d %s' % (case, _cus(), ' '.join(sorted(C.paths(case, _cus())['tags']))))
    r64, r32 = C.reference_xf(case, 'float64', option), C.reference_xf(case, 'float32', option)
    S, seg, K, Co, G = c['S'], c['seg'], c['K'], c['Co'], c['G']
    bn1 = _bn_module(K, c['gamma1'], c['beta1'], c['mean1'], c['var1'], c['train'])
    bn2 = _bn_module(Co, c['gamma'], c['beta'], c['mean'], c['var'], c['train'])
    leaves = {'y': c['y'].cuda(), 'gamma1': bn1.weight, 'beta1': bn1.bias, 'W': c['W'].cuda(), 'b': c['b'].cuda(),
              'gamma': bn2.weight, 'beta': bn2.bias}
    for k, t in leaves.items():
        t.requires_grad_(k in wrt)
    with ops.bn_groups(G):
        out, z = ops.bn_act_pointmlp_max(leaves['y'], bn1, c['slope1'], leaves['W'], leaves['b'], bn2, c['slope'], seg,
                                         want_z=want_z, last_grad=last_grad)
        assert not want_z or z is not None
        assert last_grad or not out.requires_grad
        outs = ([(out, c['gout'].cuda())] if at_out else []) + ([(z, c['gz'].cuda())] if at_z else [])
        torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
    torch.cuda.synchronize()
    got = {'out': out.detach(), 'mean': bn2.running_mean, 'var': bn2.running_var, 'mean1': bn1.running_mean, 'var1': bn1.running_var}
    if z is not None:
        got['z'] = z.detach()
    for k, t in leaves.items():
        if k in wrt and r64['d' + k] is None:
            assert t.grad is None, 'd%s: a gradient where the reference has none' % k
        elif k in wrt:
            assert t.grad is not None, 'd' + k
            got['d' + k] = t.grad
        else:
            assert t.grad is None, 'd' + k
    got = {k: v.detach().cpu() for k, v in got.items()}
    keys = [k for k in got if k != 'db' or not c['train']]
    _bound('%s-%s' % (case, option), 'gauss', got, r64, r32, keys)
    if c['train'] and 'db' in got:
        assert float(got['db'].abs().max()) == 0.0
    assert int(bn1.num_batches_tracked) == (G if c['train'] else 0) and int(bn2.num_batches_tracked) == (G if c['train'] else 0)
    sure = r64['gap'] >= C.TAU_GAP * r64['rms']
    assert float(sure.double().mean()) >= 0.99


# ----------------------------------------------------------------------------- the grid-stride loops of the backward
@pytest.mark.parametrize('name', list(C.SPARSE_CASES))
def test_sparse_backward_grid_stride_trips(name):
    """sug_pointmlp_max_bwd_sparse called directly at sizes where a dx kernel loops: more than 4096 items of the general
    kernel, more than 4 * 8192 segments of the per-wave kernel.  dx rows that no channel picked keep their bits."""
    from sug_amd._lib import lib
    L = lib()
    c = C.sparse_case(name)
    S, seg, K, Co = c['S'], c['seg'], c['K'], c['Co']
    p = C.bwd_paths(S, seg, K, Co, _cus())
    print('pointmlp-path %s cus=%d %s trips=%d' % (name, _cus(), p['dx'], p['trips']))
    assert p['trips'] >= 2 and p['dx'] == {'general-trips': 'dx<1>:large-Co', 'per-wave-trips': 'dx_seg<1,2>'}[name], p
    a, arg, x, W = c['a'].cuda(), c['arg'].cuda(), c['x'].cuda(), c['W'].cuda()
    dx = c['dx0'].cuda()
    dW = torch.full((Co, K), float('nan'), device='cuda')
    ws = torch.empty(int(L.sug_pointmlp_max_bwd_workspace(S * seg, K, Co, seg)), device='cuda')
    assert int(arg.min()) >= 0 and int(arg.max()) < seg
    rc = L.sug_pointmlp_max_bwd_sparse(_vp(a), _vp(arg), _vp(x), K, _vp(W), S * seg, K, Co, seg, _vp(dx), K, _vp(dW), _vp(ws), _stream())
    assert rc == 0, L.sug_last_error()
    torch.cuda.synchronize()
    got = {'dx': dx.cpu(), 'dW': dW.cpu()}
    _bound(name, 'sparse', got, C.sparse_ref(c, torch.float64), C.sparse_ref(c, torch.float32))
    un = ~c['picked']
    assert int(un.sum()) > 1000
    assert torch.equal(got['dx'][un], c['dx0'][un])
