"""Plain restatements of the fused per-point MLP + max layer of sug_amd/csrc/pointmlp.hip (ops.pointmlp_max,
ops.bn_act_pointmlp_max), the case builders of tests/test_pointmlp_host.py and tests/test_gpu_pointmlp_fp64.py, and
`paths`, a restatement of the launchers' dispatch conditions.

The operation, as the kernel file's header defines it, per domain group (the rows split into G equal parts, in order):
y = x.W^T + b, train-mode BatchNorm with the group's biased variance (running buffers updated with the unbiased one, once
per group, in group order; eval mode uses the running buffers), LeakyReLU, and per (segment, channel) the row n* that is
the extreme of the PRE-BatchNorm y in the direction of gamma >= 0 (max; includes +-0) resp. gamma < 0 (min), ties to the
first row.  out = act(bn(y))[n*] by an explicit gather, so autograd routes the gradient to exactly that row.  Inputs are
upcast to `dtype`: fp64 is the reference, fp32 "the same formula in plain fp32 torch", the baseline of the bound
(adapt_cases.err / within):  err(t) = max|t - ref64| / max(max|ref64|, tiny),  err(kernel) <= 8 err(fp32 torch) + 1e-7.
Nothing at module level imports sug_amd: the module is usable on the CPU.

Two input families, both functions of the case name only:
  grid   x, W multiples of 1/2 in [-1, 1], b multiples of 1/4: every partial sum of x.W^T + b is exact in fp32, so the
         kernel's extreme and its row must equal the fp64 reference exactly, ties included.
  gauss  x ~ N(0,1), W ~ N(0,1)/sqrt(K), b ~ 0.1 N(0,1).  The routing is discontinuous at near-ties, so the probe gout is
         zeroed at every (segment, channel) whose fp64 top-1 to top-2 gap is below TAU_GAP * rms(y) (about 100 times the
         fp32 error of y at K = 128).  Nothing is excluded from any comparison.
In both families gout is also zeroed where |bn(y)[n*]| < TAU_KINK * max(1, rms(bn(y)[n*])): the derivative of
LeakyReLU jumps at 0 and the BatchNorm output is not exact even on the grid.  That share is of the order 1e-4.

Planted rows, in every segment: a dominant row, DOMINANT x another row of the segment, at in-segment position p1, and an
exact copy of it at p2 > p1 in another 32-row tile (segments of one tile: another row, in half of the patterns in the other
lane half of the accumulator tile; segments of >= 1024 rows: at least seg/8 rows later, i.e. in another part of a split
segment).  x is built by indexing unique rows, and the references take the extreme over y[index]: duplicates are exactly
equal there too, so p1 wins and p2 never does.  DOMINANT is 16, not 3: a row 3 u beats the maximum of the other rows
(2.0 sigma of 31 rows, 3.2 sigma of 1023) in only P(u > max/3) = 25 % resp. 14 % of the channels (measured on these cases:
9 to 29 % per segment), short of the 25 % per segment the host tests ask for; at 16 it is 28 to 49 %, so dozens of channels
of one 64-lane ballot pick the same row (the batched weight-row loads of dx_seg, the compacted channel lists).  16 x stays
exact on the grid (|x| <= 16 + 8, sums below 2^12 in multiples of 1/4).

The dominant row is never the first row of a domain group.  y of that row is the pivot about which the kernel takes its
BatchNorm sums (common.h), which assumes a typical row: with a 16-sigma outlier there the fp32 sums about it lose
(pivot - mean)^2 / var ~ 100 times the precision (measured with the dominant row at row 0: running_var off by 1e-5 to
4e-5 of its largest value, 50 to 100 times plain fp32 torch, on grid and gauss alike).  A common offset of the data, the
case the pivot exists for, is the x + 8 variant of `partial` and `split`.

gamma has mixed signs; channels 3 and Co - 2 are exactly 0.0 and channel 70 is -0.0 (max direction, zero coefficient)."""
import functools
import math
import zlib

import torch

TINY = 1e-30
FACTOR, FLOOR = 8.0, 1e-7           # the bound of adapt_cases
TAU_GAP, TAU_KINK = 1e-4, 1e-4
DOMINANT = 16.0
EPS, MOMENTUM = 1e-5, 0.1
STATS_ROWS = 1024 - 8               # SUG_STATS_ROWS (sug_amd/csrc/common.h)
CHUNK_ELEMS = 1 << 23               # [rows, Co] elements of y alive at a time


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _spec(S, seg, K, Co, G=1, train=True, bias=True, slope=0.0, slope1=0.0):
    return dict(S=S, seg=seg, K=K, Co=Co, G=G, train=train, bias=bias, slope=slope, slope1=slope1)


CASES = {
    'tiles1': _spec(1, 32, 64, 128), 'tiles2': _spec(2, 32, 64, 128), 'tiles3': _spec(3, 32, 64, 128),
    'tiles4': _spec(4, 32, 64, 128), 'tiles5': _spec(5, 32, 64, 128),
    'partial': _spec(40, 32, 128, 128),
    'groups': _spec(80, 32, 128, 128, G=2, bias=False),
    'seg64a': _spec(24, 64, 64, 256, slope=0.2),
    'seg64b': _spec(16, 64, 128, 256, train=False),
    'seg96': _spec(6, 96, 64, 128, bias=False, slope=0.2),
    'seg128': _spec(8, 128, 128, 256, G=2),
    'split': _spec(2, 1024, 128, 512),
    'split384': _spec(4, 1024, 64, 384, G=2),
    'xcd': _spec(256, 32, 64, 128, train=False),
    'seg2048': _spec(2, 2048, 64, 128),
    'whole1024': _spec(128, 1024, 64, 512),
}
XF_CASES = {
    'xf_sa1': _spec(40, 32, 64, 128, G=2),
    'xf_sa2': _spec(16, 64, 128, 256, train=False, slope1=0.2),
    'xf_split': _spec(2, 1024, 128, 512),
}
GAUSS_ONLY = ('whole1024',)
FAMILIES = ('grid', 'gauss')
SHIFTED = ('partial', 'split')          # the grid family again with x + 8: what the pivoted BatchNorm sums exist for
SPARSE_CASES = {'general-trips': dict(S=4100, seg=32, K=64, Co=384), 'per-wave-trips': dict(S=32772, seg=32, K=64, Co=128)}


def case_list():
    """[(case, family, shift)] of ops.pointmlp_max."""
    out = [(c, f, 0.0) for c in CASES for f in FAMILIES if not (f == 'grid' and c in GAUSS_ONLY)]
    return out + [(c, 'grid', 8.0) for c in SHIFTED]


# ----------------------------------------------------------------------------- the launchers' conditions
def _dw_chunks(S):
    nsc = min(S // 16, 1024)
    if nsc < 256:
        nsc = S if S < 256 else 256
    return max(nsc, 1)


def bwd_paths(S, seg, K, Co, cu_count):
    """sug_pointmlp_max_bwd_sparse for S segments (of one domain group) -> {'dx', 'chunks', 'trips', 'nsc'}."""
    kv = K // 64
    if seg <= 64 and Co <= 256:
        grid = (S + 3) // 4 if S // 4 < 8192 else 8192
        return {'dx': 'dx_seg<%d,%d>' % (kv, 2 if Co <= 128 else 4), 'chunks': 1, 'trips': -(-S // (4 * grid)), 'nsc': _dw_chunks(S)}
    chunks = -(-seg // 128)
    while S * chunks < 2 * cu_count and seg // (chunks * 2) >= 16:
        chunks *= 2
    return {'dx': 'dx<%d>:%s' % (kv, 'small-Co' if Co <= 256 else 'large-Co'), 'chunks': chunks,
            'trips': -(-S * chunks // 4096), 'nsc': _dw_chunks(S)}


def paths(case, cu_count):
    """What case `case` reaches on a device of cu_count compute units: pointmlp_max_fwd's row blocking, split and block
    mapping, the dx kernel sug_pointmlp_max_bwd_sparse picks -> a dict with a set of 'tags' among its entries."""
    c = CASES.get(case) or XF_CASES[case]
    S, seg, K, Co, G = c['S'], c['seg'], c['K'], c['Co'], c['G']
    sg, rg = S // G, S * seg // G
    rpw = seg if seg >= 1024 else (1024 // seg) * seg
    while -(-rg // rpw) > STATS_ROWS:
        rpw *= 2
    nrb, parts = -(-rg // rpw), 1
    if rpw == seg:
        while parts < 8 and sg * parts * (Co // 128) < 2 * cu_count and seg % (parts * 2 * 128) == 0 and 2 * sg * parts * 2 <= STATS_ROWS:
            parts *= 2
        if parts > 1:
            rpw, nrb = seg // parts, sg * parts
    last = rg - (nrb - 1) * rpw
    p = {'rpw': rpw, 'nrb': nrb, 'parts': parts, 'tiles': min(rpw, rg) // 32, 'last_tiles': last // 32}
    p.update(bwd_paths(sg, seg, K, Co, cu_count))
    xf = case in XF_CASES
    tags = {'fwd<%d%s>' % (K, ',xf' if xf else ''), 'tiles=%d' % p['tiles'], p['dx'], 'train' if c['train'] else 'eval',
            'map:xcd' if nrb % 8 == 0 else 'map:linear', 'G=%d' % G}
    if p['dx'].startswith('dx<'):
        tags.add('%s:chunks=%d' % (p['dx'], p['chunks']))
    if parts > 1:
        tags.add('split:parts=%d' % parts)
        tags.add(p['dx'] + ':split')
    else:
        if nrb % 8 == 0:
            tags.add('map:xcd:unsplit')
        if seg == 1024:
            tags.add('unsplit:seg=1024')
    if nrb > 1 and last < rpw:
        tags.add('partial-last-wg')
    if seg > 32 and rpw > seg and rpw % seg == 0 and min(rpw, rg) > seg:
        tags.add('segment-ends-inside-wg')
    if seg > 1024:
        tags.add('seg>1024')
    if Co % 128 == 0 and Co & (Co - 1):
        tags.add('Co-not-pow2')
    if xf and parts > 1:
        tags.add('xf:split')
    p['tags'] = tags
    return p


# every instantiation and branch the case table names (at 256 compute units)
REQUIRED_TAGS = ['fwd<64>', 'fwd<128>', 'fwd<64,xf>', 'fwd<128,xf>', 'tiles=1', 'tiles=2', 'tiles=3', 'tiles=4', 'tiles=5',
                 'partial-last-wg', 'G=2', 'eval', 'dx_seg<1,2>', 'dx_seg<2,2>', 'dx_seg<1,4>', 'dx_seg<2,4>',
                 'dx<1>:small-Co', 'dx<1>:small-Co:chunks=4', 'dx<2>:small-Co', 'dx<2>:large-Co', 'dx<1>:large-Co',
                 'split:parts=8', 'dx<2>:large-Co:split', 'dx<1>:large-Co:split', 'Co-not-pow2', 'map:xcd:unsplit', 'map:linear',
                 'seg>1024', 'unsplit:seg=1024', 'segment-ends-inside-wg', 'xf:split']


# ----------------------------------------------------------------------------- planted rows
def planted(S, seg, G=1):
    """-> (p1, p2, q) [S] long: in-segment positions of the dominant row, of its copy and of the row it is a multiple of.
    The pattern follows the segment's index inside its domain group; the first pattern does not put the dominant row at
    row 0, because y of a group's first row is the pivot of the BatchNorm sums (see the module docstring)."""
    if seg == 32:
        cands = [(5, 9), (0, 31), (0, 4), (30, 31), (12, 17)]      # (5, 9) and (12, 17): the copy in the other lane half
    else:
        step = max(32, seg // 8)
        cands = [(31, step), (0, seg - 1), (7, seg - step + 3), (0, step)]
        if seg > 64:
            cands.insert(3, (32, seg - 1))
    p1, p2, q = [], [], []
    for s in range(S):
        a, b = cands[(s % (S // G)) % len(cands)]
        r = (a + 2) % seg
        while r in (a, b):
            r = (r + 1) % seg
        p1.append(a), p2.append(b), q.append(r)
    return torch.tensor(p1), torch.tensor(p2), torch.tensor(q)


def _plant(rows_, S, seg, G):
    """rows_ [S*seg, K] unique rows -> (x with the planted rows, index [S*seg]: the row each row is a copy of)."""
    p1, p2, q = planted(S, seg, G)
    s0 = torch.arange(S) * seg
    base = rows_.clone()
    base[s0 + p1] = DOMINANT * base[s0 + q]
    index = torch.arange(S * seg)
    index[s0 + p2] = s0 + p1
    return base[index].contiguous(), index


def _gamma(Co, g):
    gam = torch.randn(Co, generator=g)
    gam[3], gam[Co - 2], gam[70] = 0.0, 0.0, -0.0
    return gam


def _layer_inputs(family, K, Co, bias, g):
    if family == 'grid':
        W = torch.randint(-2, 3, (Co, K), generator=g).float() / 2
        b = torch.randint(-4, 5, (Co,), generator=g).float() / 4
    else:
        W = torch.randn(Co, K, generator=g) / K ** 0.5
        b = torch.randn(Co, generator=g) * 0.1
    return {'W': W, 'b': b if bias else None, 'gamma': _gamma(Co, g), 'beta': torch.randn(Co, generator=g) * 0.2,
            'mean': torch.linspace(-0.2, 0.2, Co), 'var': torch.linspace(0.5, 1.5, Co)}


def _zero_probe(c, r64):
    """gout with the discontinuities of the routing (gauss) and of the activation zeroed -> (gout, zeroed share)."""
    t = r64['pre']
    bad = t.abs() < TAU_KINK * max(1.0, float(t.double().pow(2).mean().sqrt()))
    if c['family'] == 'gauss':
        bad |= r64['gap'] < TAU_GAP * r64['rms']
    return torch.where(bad, torch.zeros_like(c['gout_raw']), c['gout_raw']), float(bad.double().mean())


@functools.lru_cache(maxsize=None)
def _inputs(case, family, shift):
    c = dict(CASES[case], case=case, family=family, shift=shift)
    S, seg, K, Co = c['S'], c['seg'], c['K'], c['Co']
    g = gen('pointmlp', case, family)
    if family == 'grid':
        rows_ = torch.randint(-2, 3, (S * seg, K), generator=g).float() / 2
    else:
        rows_ = torch.randn(S * seg, K, generator=g)
    x, c['index'] = _plant(rows_, S, seg, c['G'])
    c['x'] = x + shift
    c.update(_layer_inputs(family, K, Co, c['bias'], g))
    c['gout_raw'] = torch.randn(S, Co, generator=g)
    return c


@functools.lru_cache(maxsize=None)
def build(case, family, shift=0.0):
    """One ops.pointmlp_max case: fp32 inputs, the planted positions and the probe gout (see the module docstring)."""
    c = dict(_inputs(case, family, shift))
    c['gout'], c['zeroed'] = _zero_probe(c, _ref(c, torch.float64, None))
    return c


@functools.lru_cache(maxsize=None)
def _xf_inputs(case):
    c = dict(XF_CASES[case], case=case, family='gauss', shift=0.0)
    S, seg, K, Co, G = c['S'], c['seg'], c['K'], c['Co'], c['G']
    g = gen('pointmlp-xf', case)
    y, c['index'] = _plant(torch.randn(S * seg, K, generator=g), S, seg, G)
    g1 = torch.randn(K, generator=g)
    c['gamma1'] = torch.where(g1 >= 0, g1.clamp_min(0.25), g1.clamp_max(-0.25))     # mixed signs, away from 0 (see the kink below)
    c['beta1'] = torch.randn(K, generator=g) * 0.2
    c['mean1'], c['var1'] = torch.linspace(-0.1, 0.3, K), torch.linspace(0.6, 1.4, K)
    c.update(_layer_inputs('gauss', K, Co, True, g))
    for _ in range(8):
        t1 = _bn(y.double(), c['gamma1'].double(), c['beta1'].double(), c['mean1'].double(), c['var1'].double(), G, c['train'])[0]
        near = t1.abs() < 1e-3
        if not bool(near.any()):
            break
        near |= near[c['index']]                  # a copy moves with the row it copies
        y = torch.where(near, y + 0.125, y)
        y = y[c['index']]
    else:
        raise AssertionError('could not move y off the kink')
    c['y'] = y.contiguous()
    c['gout_raw'] = torch.randn(S, Co, generator=g)
    c['gz'] = torch.randn(S * seg, K, generator=g)
    return c


@functools.lru_cache(maxsize=None)
def build_xf(case):
    """One ops.bn_act_pointmlp_max case (gauss): y [rows, K] pre-activation rows of the layer in front, its BatchNorm, and
    the last layer.  y is moved off the kink of act1 (|bn1(y)| >= 1e-3) so that z's derivative does not jump within fp32
    rounding of the reference."""
    c = dict(_xf_inputs(case))
    c['gout'], c['zeroed'] = _zero_probe(c, _ref_xf(c, torch.float64, None, None, ()))
    return c


# ----------------------------------------------------------------------------- restatements
def _act(t, slope):
    return torch.where(t > 0, t, slope * t)


def _bn(y, gamma, beta, rm, rv, G, train):
    """BatchNorm over the rows of y [rows, C] per domain group -> (bn(y), running mean, running var) (no activation)."""
    outs = []
    rg = y.shape[0] // G
    for yg in y.view(G, rg, -1):
        if train:
            mean = yg.mean(0)
            var = ((yg - mean) ** 2).mean(0)
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
            rv = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * rg / (rg - 1)
        else:
            mean, var = rm, rv
        outs.append((yg - mean) / torch.sqrt(var + EPS) * gamma + beta)
    return torch.cat(outs), rm, rv


def _seg_chunks(S, seg, Co):
    n = max(1, CHUNK_ELEMS // (seg * Co))
    return [(a, min(a + n, S)) for a in range(0, S, n)]


def route(x, W, b, gamma, seg, index):
    """The routing of the layer, without autograd -> (n* [S, Co] long, zext, gap, rms(y)).  y is taken at row index[r]
    for row r (exact copies are exactly equal); the gap is that to the best row that is no copy of the winner."""
    with torch.no_grad():
        S, Co = x.shape[0] // seg, W.shape[0]
        up = gamma >= 0
        ar = torch.arange(seg).view(1, seg, 1)
        ns, zs, gaps, ssq = [], [], [], 0.0
        for a, e in _seg_chunks(S, seg, Co):
            y = x[a * seg:e * seg] @ W.t()
            if b is not None:
                y = y + b
            y = y[index[a * seg:e * seg] - a * seg].view(e - a, seg, Co)
            ssq += float((y.double() ** 2).sum())
            f = torch.where(up, y, -y)
            top = f.max(dim=1).values
            n = torch.where(f == top.unsqueeze(1), ar, seg).min(dim=1).values            # the first row at the extreme
            bid = index[a * seg:e * seg].view(e - a, seg)
            same = bid.unsqueeze(2) == bid.gather(1, n).unsqueeze(1)
            second = f.masked_fill(same, -math.inf).max(dim=1).values
            ns.append(n), zs.append(torch.where(up, top, -top)), gaps.append(top - second)
        return torch.cat(ns), torch.cat(zs), torch.cat(gaps), math.sqrt(ssq / (S * seg * Co))


def layer(x, W, b, gamma, beta, rm, rv, slope, seg, G, train, nstar):
    """Differentiable part: -> (out [S, Co], bn(y)[n*], running mean, running var) for the given rows n* [S, Co]."""
    S, Co = x.shape[0] // seg, W.shape[0]
    sg, rg = S // G, x.shape[0] // G
    pres = []

    def y_of(xg, a, e):
        y = xg[a * seg:e * seg] @ W.t()
        return y if b is None else y + b

    for gi in range(G):
        xg, ng = x[gi * rg:(gi + 1) * rg], nstar[gi * sg:(gi + 1) * sg]
        chunks = _seg_chunks(sg, seg, Co)
        s1, ysel = 0.0, []
        for a, e in chunks:
            y = y_of(xg, a, e)
            s1 = s1 + y.sum(0)
            ysel.append(y.view(e - a, seg, Co).gather(1, ng[a:e].unsqueeze(1)).squeeze(1))     # y[n*]: an explicit gather
        ysel = torch.cat(ysel)
        if train:
            mean = s1 / rg
            var = sum(((y_of(xg, a, e) - mean) ** 2).sum(0) for a, e in chunks) / rg
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
            rv = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * rg / (rg - 1)
        else:
            mean, var = rm, rv
        pres.append((ysel - mean) / torch.sqrt(var + EPS) * gamma + beta)      # elementwise: bn(y)[n*] = bn(y[n*])
    pre = torch.cat(pres)
    return _act(pre, slope), pre, rm, rv


def pointmlp_max_ref(x, W, b, gamma, beta, bn_state, slope, seg, G, train, dtype, index=None, probe=None, nstar=None):
    """bn_state = (running_mean, running_var).  index [rows]: the row each row is an exact copy of (default: itself).
    nstar: a fixed routing (the gradcheck of the host tests).  -> dict: out, nstar, zext, gap, rms, pre (= bn(y)[n*]),
    mean, var (the updated running buffers), and dx, dW, db, dgamma, dbeta for the probe (a gradient of out)."""
    x, W, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, W, gamma, beta))
    b = None if b is None else b.detach().to(dtype).clone().requires_grad_(True)
    rm, rv = (t.to(dtype) for t in bn_state)
    index = torch.arange(x.shape[0]) if index is None else index
    n, zext, gap, rms = route(x.detach(), W.detach(), None if b is None else b.detach(), gamma.detach(), seg, index)
    out, pre, rm, rv = layer(x, W, b, gamma, beta, rm, rv, slope, seg, G, train, n if nstar is None else nstar)
    r = {'out': out.detach(), 'nstar': n, 'zext': zext, 'gap': gap, 'rms': rms, 'pre': pre.detach(), 'mean': rm, 'var': rv}
    if probe is not None:
        wrt = {'dx': x, 'dW': W, 'dgamma': gamma, 'dbeta': beta}
        if b is not None:
            wrt['db'] = b
        r.update(zip(wrt, torch.autograd.grad(out, list(wrt.values()), probe.to(dtype))))
    return r


def bn_act_pointmlp_max_ref(y, gamma1, beta1, bn1_state, slope1, W, b, gamma, beta, bn_state, slope, seg, G, train, dtype,
                            index=None, probe=None, probe_z=None, wrt=('y', 'gamma1', 'beta1', 'W', 'b', 'gamma', 'beta'),
                            nstar=None):
    """The same with z = act1(bn1(y)) in front, per group.  probe / probe_z: the gradients arriving at out / at z (None:
    none arrives); wrt: the inputs that take a gradient.  -> the dict of pointmlp_max_ref plus z, mean1, var1 and
    'd' + name for every name of wrt (None where no gradient reaches it)."""
    leaves = {'y': y, 'gamma1': gamma1, 'beta1': beta1, 'W': W, 'b': b, 'gamma': gamma, 'beta': beta}
    t = {k: None if v is None else v.detach().to(dtype).clone().requires_grad_(k in wrt) for k, v in leaves.items()}
    rm1, rv1 = (v.to(dtype) for v in bn1_state)
    rm, rv = (v.to(dtype) for v in bn_state)
    index = torch.arange(y.shape[0]) if index is None else index
    pre1, rm1, rv1 = _bn(t['y'], t['gamma1'], t['beta1'], rm1, rv1, G, train)
    z = _act(pre1, slope1)
    bd = None if b is None else t['b'].detach()
    n, zext, gap, rms = route(z.detach(), t['W'].detach(), bd, t['gamma'].detach(), seg, index)
    out, pre, rm, rv = layer(z, t['W'], t['b'], t['gamma'], t['beta'], rm, rv, slope, seg, G, train, n if nstar is None else nstar)
    r = {'out': out.detach(), 'z': z.detach(), 'nstar': n, 'zext': zext, 'gap': gap, 'rms': rms, 'pre': pre.detach(),
         'mean': rm, 'var': rv, 'mean1': rm1, 'var1': rv1}
    outs = [(o, p.to(dtype)) for o, p in ((out, probe), (z, probe_z)) if p is not None]
    names = [k for k in wrt if t[k] is not None]
    if outs and names:
        grads = torch.autograd.grad([o for o, _ in outs], [t[k] for k in names], [p for _, p in outs], allow_unused=True)
        r.update(('d' + k, v) for k, v in zip(names, grads))
    return r


def _ref(c, dtype, probe):
    return pointmlp_max_ref(c['x'], c['W'], c['b'], c['gamma'], c['beta'], (c['mean'], c['var']), c['slope'], c['seg'], c['G'],
                            c['train'], dtype, index=c['index'], probe=probe)


def _ref_xf(c, dtype, probe, probe_z, wrt):
    return bn_act_pointmlp_max_ref(c['y'], c['gamma1'], c['beta1'], (c['mean1'], c['var1']), c['slope1'], c['W'], c['b'],
                                   c['gamma'], c['beta'], (c['mean'], c['var']), c['slope'], c['seg'], c['G'], c['train'],
                                   dtype, index=c['index'], probe=probe, probe_z=probe_z, wrt=wrt)


@functools.lru_cache(maxsize=None)
def reference(case, family, shift, dtype):
    """pointmlp_max_ref of a case in 'float64' or 'float32', computed once per process and shared; read-only."""
    c = build(case, family, shift)
    return _ref(c, getattr(torch, dtype), c['gout'])


XF_OPTIONS = {
    # name: (want_z, a gradient arrives at out, one arrives at z, last_grad, the inputs that take a gradient)
    'plain': (False, True, False, True, ('y', 'gamma1', 'beta1', 'W', 'b', 'gamma', 'beta')),
    'want_z': (True, True, False, True, ('y', 'gamma1', 'beta1', 'W', 'b', 'gamma', 'beta')),
    'grad_at_z': (True, True, True, True, ('y', 'gamma1', 'beta1', 'W', 'b', 'gamma', 'beta')),
    'z_only': (True, False, True, False, ('y', 'gamma1', 'beta1', 'W', 'b', 'gamma', 'beta')),
    'last_frozen': (False, True, False, True, ('y', 'gamma1', 'beta1')),
    'y_fixed': (True, True, True, True, ('gamma1', 'beta1', 'W', 'b', 'gamma', 'beta')),
}


@functools.lru_cache(maxsize=None)
def reference_xf(case, dtype, option):
    """bn_act_pointmlp_max_ref of an XF case under one of XF_OPTIONS, computed once per process and shared; read-only."""
    _, at_out, at_z, _, wrt = XF_OPTIONS[option]
    c = build_xf(case)
    return _ref_xf(c, getattr(torch, dtype), c['gout'] if at_out else None, c['gz'] if at_z else None, wrt)


def err(x, ref):
    ref = ref.double()
    if ref.numel() == 0:
        return 0.0
    return float((x.detach().double().cpu() - ref).abs().max() / max(float(ref.abs().max()), TINY))


def within(ek, e32, factor=FACTOR):
    return ek <= factor * e32 + FLOOR


# ----------------------------------------------------------------------------- the sparse backward on its own
def sparse_case(name):
    """Inputs of sug_pointmlp_max_bwd_sparse called directly: a ~ N(0,1), arg uniform in [0, seg); in every 16th segment half
    of the channels pick the planted row p1 and the rest one of rows 0..7, so that rows nobody picked exist.  dx0: what dx
    holds before the call (the kernel adds into the rows that were picked and leaves the others alone)."""
    c = dict(SPARSE_CASES[name])
    S, seg, K, Co = c['S'], c['seg'], c['K'], c['Co']
    g = gen('pointmlp-sparse', name)
    arg = torch.randint(0, seg, (S, Co), generator=g)
    p1 = planted(S, seg)[0]
    plant = torch.rand(S, Co, generator=g) < 0.5
    few = torch.randint(0, 8, (S, Co), generator=g)
    every16 = (torch.arange(S) % 16 == 0).view(S, 1)
    arg = torch.where(every16, torch.where(plant, p1.view(S, 1).expand(S, Co), few), arg)
    c.update(a=torch.randn(S, Co, generator=g), arg=arg.to(torch.int32), x=torch.randn(S * seg, K, generator=g),
             W=torch.randn(Co, K, generator=g) / K ** 0.5, dx0=torch.randn(S * seg, K, generator=g))
    picked = torch.zeros(S * seg, dtype=torch.bool)
    picked[(torch.arange(S).view(S, 1) * seg + arg).flatten()] = True
    c['picked'] = picked
    return c


def sparse_ref(c, dtype):
    """dx = dx0 + index_add of a[s,c] W[c,:] at row s seg + arg[s,c];  dW[c,:] = sum_s a[s,c] x[s seg + arg[s,c], :]; in
    segment chunks."""
    S, seg, K, Co = c['S'], c['seg'], c['K'], c['Co']
    a, W, x = c['a'].to(dtype), c['W'].to(dtype), c['x'].to(dtype)
    dx, dW = c['dx0'].to(dtype).clone(), torch.zeros(Co, K, dtype=dtype)
    n = max(1, (1 << 24) // (Co * K))
    for s0 in range(0, S, n):
        s1 = min(s0 + n, S)
        rows_ = (torch.arange(s0, s1).view(-1, 1) * seg + c['arg'][s0:s1].long())
        dx.index_add_(0, rows_.flatten(), (a[s0:s1].unsqueeze(2) * W.unsqueeze(0)).view(-1, K))
        dW += torch.einsum('sc,sck->ck', a[s0:s1], x[rows_])
    return {'dx': dx, 'dW': dW}
