"""The EdgeConv layer and the two-layer block at B = 2, N = 2048, k = 20, Co = 64 (40 960 entries per cloud: the reverse
lists of the backward come from the tiled build), for tests/test_edgeconv_large_host.py and
tests/test_gpu_edgeconv_large.py.  Restatements, error measure and bound are those of tests/dgcnn_seg_cases.py (DESIGN 4b:
err(kernel) <= 8 err(the same formula in fp32 torch) + 1e-7 against fp64); nothing here imports sug_amd.

Neighbour lists: dgcnn_seg_cases.lists (random with repeats; point HUB named by every list twice, a dominant row and its
exact copy at a later j; point N - 1 named by none) and a second hub, point HUB2, in column 0 of the lists of the first
N / 2 points wherever column 0 is not the first hub's.  The points N - 1 and N - 2 are named by nobody.

Margins.  5.2 million first-layer activations cannot all be drawn KINK1 away from LeakyReLU's kink (dgcnn_seg_cases redraws
until they are: at this size 8 of them are expected inside it whatever the seed).  The probe is zeroed instead wherever the
gradient would pass such an element: at every (point, channel) whose winning edge holds a first-layer value within KINK1 of
the kink, besides the block-level rules of dgcnn_seg_cases.block_case (pre-activation of the winner within TAU_KINK of the
kink, top-1 to top-2 gap below TAU_GAP rms, copies of the winner aside).  Through a losing edge only the BatchNorm mean
terms flow, 1 / (B N k) of a winner's.  At most MAX_ZEROED of the pairs may be zeroed."""
import functools

import torch
import torch.nn.functional as F

import dgcnn_seg_cases as D
from oracle import ref_cpu as O

B, N, K, CO = 2, 2048, 20, 64
HUB2 = 7
SLOPE = 0.2
LAYER_GRADS = ('x', 'W', 'gamma', 'beta')


@functools.lru_cache(maxsize=None)
def inputs():
    """x [B,3,N], idx [B,N,k] long, the block's parameters (dgcnn_seg_cases._params, Co = 64: LeakyReLU(0.2), no biases),
    the layer's (W [64,6], gamma of mixed sign, beta, running buffers) and one probe gout [B,Co,N]."""
    g = D.gen('edgeconv-large')
    x = torch.randn(B, 3, N, generator=g)
    x[:, :, D.HUB] = D.DOMINANT * x[:, :, D.HUB + 1]
    idx, j1, j2 = D.lists(B, N, K, g)
    idx = torch.where(idx == N - 2, torch.full_like(idx, N - 3), idx)              # N - 2 joins N - 1: named by nobody
    first = torch.arange(N // 2)
    first = first[j1[: N // 2] != 0]
    idx[:, first, 0] = HUB2
    p = D._params(CO, g)
    gl = torch.randn(CO, generator=g)
    layer = {'W': torch.randn(CO, 6, generator=g) / 6 ** 0.5, 'gamma': torch.where(gl >= 0, gl.clamp_min(0.25), gl.clamp_max(-0.25)),
             'beta': torch.randn(CO, generator=g) * 0.2, 'mean': torch.linspace(-0.1, 0.3, CO), 'var': torch.linspace(0.6, 1.4, CO)}
    return {'x': x, 'idx': idx, 'p': p, 'layer': layer, 'gout': torch.randn(B, CO, N, generator=g)}


def layer_forward(x, q, idx, nstar=None):
    """One EdgeConv layer in train mode: e = graph_feature(x, idx); y = conv(e, W); per (point, channel) the first j at the
    extreme of y in the direction of gamma; out = LeakyReLU(bn(y))[j*] by an explicit gather."""
    y = F.conv2d(O.graph_feature(x, K, idx), q['W'].view(CO, 6, 1, 1))
    n, zext, gap, rms = D.route(y.detach(), q['gamma'].detach(), idx)
    t, rm, rv = D._bn(y, q['gamma'], q['beta'], q['mean'], q['var'], True)
    pre = t.gather(3, (n if nstar is None else nstar).unsqueeze(3)).squeeze(3)
    return {'out': D.act(pre, SLOPE), 'pre': pre, 'nstar': n, 'gap': gap, 'rms': rms, 'mean': rm, 'var': rv}


def _near(t, tau):
    return t.abs() < tau * max(1.0, float(t.pow(2).mean().sqrt()))


@functools.lru_cache(maxsize=None)
def probes():
    """(layer probe, block probe, the shares zeroed): gout with the pairs zeroed that the margins exclude, from the fp64
    forwards."""
    c = inputs()
    with torch.no_grad():
        r = layer_forward(c['x'].double(), D._cast(c['layer'], torch.float64), c['idx'])
        bad_l = _near(r['pre'], D.TAU_KINK) | (r['gap'] < D.TAU_GAP * r['rms'])
        r = D.block(c['x'].double(), D._cast(c['p'], torch.float64), c['idx'], True)
        bad_b = _near(r['pre'], D.TAU_KINK) | (r['gap'] < D.TAU_GAP * r['rms'])
        edge = (r['t1'].abs() < D.KINK1).any(dim=1)                                                # [B,N,k]
        bad_b |= edge.unsqueeze(1).expand(B, CO, N, K).gather(3, r['nstar'].unsqueeze(3)).squeeze(3)
    zero = torch.zeros_like(c['gout'])
    return (torch.where(bad_l, zero, c['gout']), torch.where(bad_b, zero, c['gout']),
            (float(bad_l.double().mean()), float(bad_b.double().mean())))


@functools.lru_cache(maxsize=None)
def layer_reference(dtype):
    """The layer restatement in 'float64' / 'float32' with the gradients of its probe; shared, read-only."""
    c, dt = inputs(), getattr(torch, dtype)
    q = D._cast(c['layer'], dt)
    for n in LAYER_GRADS[1:]:
        q[n].requires_grad_(True)
    x = c['x'].to(dt).clone().requires_grad_(True)
    r = layer_forward(x, q, c['idx'])
    grads = torch.autograd.grad(r['out'], [x] + [q[n] for n in LAYER_GRADS[1:]], probes()[0].to(dt))
    res = {k_: (v.detach() if torch.is_tensor(v) else v) for k_, v in r.items()}
    res.update({'d' + n: gr for n, gr in zip(LAYER_GRADS, grads)})
    return res


@functools.lru_cache(maxsize=None)
def block_reference(dtype):
    """dgcnn_seg_cases.block in train mode in 'float64' / 'float32' with the gradients of the block probe."""
    c, dt = inputs(), getattr(torch, dtype)
    p = D._cast(c['p'], dt, grad=True)
    x = c['x'].to(dt).clone().requires_grad_(True)
    r = D.block(x, p, c['idx'], True)
    leaves = {'x': x, **{n: p[n] for n in D.GRAD_NAMES[1:] if p[n] is not None}}
    grads = torch.autograd.grad(r['out'], list(leaves.values()), probes()[1].to(dt))
    res = {k_: (v.detach() if torch.is_tensor(v) else v) for k_, v in r.items() if k_ in ('out', 'pre', 'nstar', 'mean1', 'var1',
                                                                                         'mean2', 'var2', 't1')}
    res.update({'d' + n: gr for n, gr in zip(leaves, grads)})
    return res
