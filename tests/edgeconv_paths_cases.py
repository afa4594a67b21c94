"""The single EdgeConv layer (sug_amd/csrc/edgeconv.hip, edgeconv_fused.hip; ops.edgeconv_bn_act_max, ops.edgeconv_fused,
conv_2d.edge_rows) on every dispatch path, for tests/test_edgeconv_paths_host.py and tests/test_gpu_edgeconv_paths.py.
Restatement pieces, error measure and bound are those of tests/dgcnn_seg_cases.py (err(kernel) <= 8 err(the
same formula in fp32 torch) + 1e-7 against fp64); nothing at module level imports sug_amd.

The layer, per domain group of B / G clouds with statistics of their own (the groups take the running buffers one after
the other, as separate BatchNorm calls would):  y = conv(graph_feature(x, idx), W, b) [Bg,Co,N,k];  per (point, channel)
the FIRST j at the extreme of y in the direction of gamma (dgcnn_seg_cases.route);  out = act(bn(y))[j*] by an explicit
gather, so that autograd routes the gradient to exactly that edge.

Inputs of a case (seeded by its name): x [B,C,N] with x[:, :, HUB] = DOMINANT * x[:, :, HUB + 1]; idx from
dgcnn_seg_cases.lists (random with repeats; point HUB named by every list twice, the second time as an exact copy at a later
j; point N - 1 named by no list); W [Co,2C] / sqrt(2C); gamma of mixed sign with |gamma| >= 0.25; beta; running buffers off
their defaults; an optional conv bias; one probe gout [B,Co,N].  The probe is zeroed where the fp64 |pre| lies within
TAU_KINK * max(1, rms(pre)) of the activation's kink and where the top-1 to top-2 gap, copies of the winner aside, is
below TAU_GAP * rms(y) of the group; at most MAX_ZEROED of the pairs may be zeroed (a condition on the seed).

CASES holds the smallest shapes at which each kernel, template instance and regime of the dispatch exists -- `reaches`
says which, EXPECT states it as numbers that test_edgeconv_paths_host.py holds against the library (ops.edgeconv_path,
ops.edgeconv_fused_supported) and against the launch arithmetic restated below."""
import functools

import torch
import torch.nn.functional as F

import dgcnn_seg_cases as D
from oracle import ref_cpu as O

# slope: the fused cases run through conv_2d('leakyrelu') = nn.LeakyReLU() (0.01), the others call the op with DGCNN's 0.2
FUSED_SLOPE, OP_SLOPE = 0.01, 0.2

#  name: (B, N, k, C, Co, groups, bias, train)
CASES = {
    'fused-c3': (2, 96, 20, 3, 64, 1, False, True),                 # fused CIN = 4, QLDS; LDS backward
    'fused-c64-groups-bias': (4, 96, 20, 64, 64, 2, True, True),    # fused CIN = 64, two groups, bias on Q
    'fused-c128': (2, 64, 20, 128, 32, 1, False, True),             # fused CIN = 128 (ops.EDGECONV_FUSED_MAXC = 128)
    'fused-q-global': (1, 1280, 20, 3, 16, 1, False, True),         # fused QLDS = false; generic backward <1,20>; hub fan-in > 2N
    'fused-eval': (2, 96, 20, 64, 32, 1, True, False),              # sug_affine_act_groups tail, eval backward, db
    'lds-psplit4': (3, 100, 20, 8, 48, 1, False, True),             # GEMM path, LDS forward and backward, psplit 4
    'lds-xcd': (8, 40, 20, 8, 16, 2, False, True),                  # LDS backward XCD remap with groups
    'lds-two-pass': (1, 1040, 20, 8, 16, 1, False, True),           # LDS backward n_own = 260 > 256, hub list >= 255
    'lds-psplit1': (16, 40, 20, 8, 512, 1, False, True),            # psplit 1 both ways
    'lds-eval': (2, 100, 20, 8, 32, 2, False, False),               # per-group sug_edgeconv_fwd + sug_affine_act loop
    'gen-k7-co12': (3, 70, 7, 8, 12, 1, True, True),                # generic <1> / <1,0>, Co/4 = 3 of 4 lanes
    'gen-k20-co40': (2, 70, 20, 8, 40, 2, False, True),             # generic forward at k = 20, <1,20> per group
    'gen-nch2': (2, 40, 5, 8, 320, 1, False, True),                 # <2>, partial second chunk
    'gen-nch3': (1, 40, 5, 8, 768, 1, False, True),                 # nch = 3 launched as <4>
    'gen-nch4': (1, 40, 5, 8, 1024, 1, False, True),                # <4> full
    'gen-k255': (1, 64, 255, 8, 16, 1, False, True),                # largest k for the uint8 arg
    'gen-n2304': (1, 2304, 20, 8, 16, 1, False, True),              # past the LDS forward (N > 2272); tiled reverse lists
    'gen-eval': (2, 70, 7, 8, 12, 1, False, False),                 # generic eval backward
}
FIELDS = ('B', 'N', 'k', 'C', 'Co', 'G', 'bias', 'train')

# What a case reaches: fused (conv_2d.edge_rows takes the fused layer; maxc: only with ops.EDGECONV_FUSED_MAXC = 128),
# qlds (Q slice in LDS), fwd / bwd ('lds' | 'generic': ops.edgeconv_path; fwd None for the fused layer), nch (float4 chunks
# per lane of the generic kernels, 3 is launched as <4>), pf / pb (psplit of the LDS forward / backward), n_own (points of
# part 0 of the LDS backward; its 1024 threads visit 256 per pass).
EXPECT = {
    'fused-c3': dict(fused=True, qlds=True, bwd='lds', pb=4),
    'fused-c64-groups-bias': dict(fused=True, qlds=True, bwd='lds', pb=4),
    'fused-c128': dict(fused=True, maxc=True, qlds=True, bwd='lds', pb=4),
    'fused-q-global': dict(fused=True, qlds=False, bwd='generic', nch=1),
    'fused-eval': dict(fused=True, qlds=True, bwd='lds', pb=4),
    'lds-psplit4': dict(fused=False, fwd='lds', bwd='lds', pf=4, pb=4),
    'lds-xcd': dict(fused=False, fwd='lds', bwd='lds', pf=4, pb=4, xcd=True),
    'lds-two-pass': dict(fused=False, fwd='lds', bwd='lds', pf=4, pb=4, n_own=260),
    'lds-psplit1': dict(fused=False, fwd='lds', bwd='lds', pf=1, pb=1, xcd=True),
    'lds-eval': dict(fused=False, fwd='lds', bwd='lds', pf=4, pb=4),
    'gen-k7-co12': dict(fused=False, fwd='generic', bwd='generic', nch=1),
    'gen-k20-co40': dict(fused=False, fwd='generic', bwd='generic', nch=1),
    'gen-nch2': dict(fused=False, fwd='generic', bwd='generic', nch=2),
    'gen-nch3': dict(fused=False, fwd='generic', bwd='generic', nch=3),
    'gen-nch4': dict(fused=False, fwd='generic', bwd='generic', nch=4),
    'gen-k255': dict(fused=False, fwd='generic', bwd='generic', nch=1),
    'gen-n2304': dict(fused=False, fwd='generic', bwd='generic', nch=1),
    'gen-eval': dict(fused=False, fwd='generic', bwd='generic', nch=1),
}
GRADS = ('x', 'W', 'gamma', 'beta')


def shape(name):
    return dict(zip(FIELDS, CASES[name]))


# ----------------------------------------------------------------------------- the launch arithmetic, restated
def generic_nch(Co):
    """float4 chunks per lane of edgeconv_fwd_kernel / edgeconv_bwd_scatter_kernel (lanes_per_point in edgeconv.hip)."""
    lpp = 1
    while lpp < Co // 4 and lpp < 64:
        lpp *= 2
    return (Co // 4 + lpp - 1) // lpp


def lds_psplit(backward, B, Co):
    """Parts a cloud's points are cut into by edgeconv_fwd_lds_kernel (512 workgroups aimed at) / edgeconv_bwd_lds_kernel (256)."""
    return min(max((256 if backward else 512) // (B * (Co // 16)), 1), 4)


def lds_n_own(N, psplit):
    """Destination points of part 0 of the LDS backward (a part owns the points m = part mod psplit)."""
    return (N + psplit - 1) // psplit


def fused_qlds(N):
    """launch_fused in edgeconv_fused.hip: the P and Q images of a 16-channel slice and the pivot row within 160 KB."""
    return N * 16 * 4 * 2 + 2 * 16 * 4 <= 160 * 1024


# ----------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(name):
    """x [B,C,N], idx [B,N,k] long, W, b (or None), gamma, beta, mean, var, gout [B,Co,N]; shared, read-only."""
    s = shape(name)
    B, N, k, C, Co = s['B'], s['N'], s['k'], s['C'], s['Co']
    g = D.gen('edgeconv-paths', name)
    x = torch.randn(B, C, N, generator=g)
    x[:, :, D.HUB] = D.DOMINANT * x[:, :, D.HUB + 1]
    idx, j1, j2 = D.lists(B, N, k, g)
    gl = torch.randn(Co, generator=g)
    c = {'x': x, 'idx': idx, 'j1': j1, 'j2': j2, 'W': torch.randn(Co, 2 * C, generator=g) / (2 * C) ** 0.5,
         'gamma': torch.where(gl >= 0, gl.clamp_min(0.25), gl.clamp_max(-0.25)), 'beta': torch.randn(Co, generator=g) * 0.2,
         'mean': torch.linspace(-0.1, 0.3, Co), 'var': torch.linspace(0.6, 1.4, Co),
         'b': torch.randn(Co, generator=g) * 0.1 if s['bias'] else None, 'gout': torch.randn(B, Co, N, generator=g),
         'slope': FUSED_SLOPE if EXPECT[name]['fused'] else OP_SLOPE}
    c.update(s)
    return c


def _near(t, tau):
    return t.abs() < tau * max(1.0, float(t.pow(2).mean().sqrt()))


def layer_forward(c, x, W, b, gamma, beta, nstar=None):
    """The layer of case c on x [B,C,N] -> dict(out [B,Co,N], pre, nstar, bad (the pairs the margins exclude), mean, var);
    nstar: route by these j instead of the restatement's own."""
    G, Co, k = c['G'], c['Co'], c['k']
    Bg = c['B'] // G
    rm, rv = c['mean'].to(x.dtype), c['var'].to(x.dtype)
    pres, ns, bads = [], [], []
    for g in range(G):
        sl = slice(g * Bg, (g + 1) * Bg)
        idg = c['idx'][sl]
        y = F.conv2d(O.graph_feature(x[sl], k, idg), W.view(Co, -1, 1, 1), b)
        n, _, gap, rms = D.route(y.detach(), gamma.detach(), idg)
        t, rm, rv = D._bn(y, gamma, beta, rm, rv, c['train'])
        pre = t.gather(3, (n if nstar is None else nstar[sl]).unsqueeze(3)).squeeze(3)          # the explicit gather
        pres.append(pre), ns.append(n)
        bads.append(_near(pre.detach(), D.TAU_KINK) | (gap < D.TAU_GAP * rms))
    pre = torch.cat(pres)
    return {'out': D.act(pre, c['slope']), 'pre': pre, 'nstar': torch.cat(ns), 'bad': torch.cat(bads), 'mean': rm, 'var': rv}


@functools.lru_cache(maxsize=None)
def probe(name):
    """(gout with the excluded pairs zeroed, the share zeroed), from the fp64 forward."""
    c = inputs(name)
    with torch.no_grad():
        cast = lambda t: None if t is None else t.double()
        r = layer_forward(c, cast(c['x']), cast(c['W']), cast(c['b']), cast(c['gamma']), cast(c['beta']))
    return torch.where(r['bad'], torch.zeros_like(c['gout']), c['gout']), float(r['bad'].double().mean())


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """The restatement in 'float64' / 'float32' with the gradients of the probe: out, pre, nstar, mean, var (the running
    buffers after the call), dx, dW, dgamma, dbeta, and db where the case has a bias; shared, read-only."""
    c, dt = inputs(name), getattr(torch, dtype)
    leaf = lambda t: t.to(dt).clone().requires_grad_(True)
    leaves = {'x': leaf(c['x']), 'W': leaf(c['W']), 'gamma': leaf(c['gamma']), 'beta': leaf(c['beta'])}
    if c['b'] is not None:
        leaves['b'] = leaf(c['b'])
    r = layer_forward(c, leaves['x'], leaves['W'], leaves.get('b'), leaves['gamma'], leaves['beta'])
    grads = torch.autograd.grad(r['out'], list(leaves.values()), probe(name)[0].to(dt))
    res = {k_: v.detach() for k_, v in r.items()}
    res.update({'d' + n: gr for n, gr in zip(leaves, grads)})
    return res


def compared(name):
    """The tensors of a case that the bound is applied to."""
    c = shape(name)
    names = ['out'] + ['d' + n for n in GRADS]
    if c['bias'] and not c['train']:
        names.append('db')                               # eval mode: the conv bias has a real gradient, colsum(dpq[:, Co:])
    if c['train']:
        names += ['mean', 'var']
    return names
