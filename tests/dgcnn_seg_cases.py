"""Plain-torch restatements of the two-layer EdgeConv block (sug_amd/csrc/edgemlp.hip, ops.edgeconv2) and of
model/dgcnn_seg.DGCNNPartSeg, with the case builders of tests/test_dgcnn_seg_host.py, tests/test_gpu_edgemlp.py and
tests/test_gpu_dgcnn_seg.py.  Nothing at module level imports sug_amd: the module is usable on the CPU.

The block, from the pieces the DGCNN goldens pin (oracle.ref_cpu.graph_feature, conv_bn_act / its BatchNorm, transform_net's
layers):  e = graph_feature(x, idx) [B,2C,N,k];  y1 = conv(e, W1) (+ b1);  a1 = LeakyReLU_s1(bn1(y1));  y2 = conv(a1, W2)
(+ b2); per (point, channel) the FIRST j at the extreme of the pre-BatchNorm y2 in the direction of gamma2 >= 0 (max,
includes +-0) resp. gamma2 < 0 (min); out = LeakyReLU_s2(bn2(y2))[j*] by an explicit gather, so that autograd
routes the gradient to exactly that edge.  Both BatchNorms take their statistics over all B*N*k values.

Bound: err(t) = max|t - ref64| / max(max|ref64|, tiny),  err(kernel) <= 8 err(the same formula in fp32 torch)
+ 1e-7.

Shapes (B, N, k, Co), C1 = 64: those of the issue.  The kernels have no grid-stride loop (a workgroup owns a fixed range of
whole segments; the row blocking is one formula), so there is no size at which a second trip starts; `straddle` and `multi`
run several workgroups, `multi` and `k2` a partial last one.

Neighbour lists: random with repeats; point HUB is named by EVERY list twice, at j1 = (i + 1) % (k - 1) and at j2 = k - 1 >
j1 -- a dominant row (x[HUB] = 16 x another point) and its exact copy at a later j; point N - 1 is named by NO list.  The
copy never wins: wherever the restatement routes to j1 the kernel's arg must be j1.

Families: `grid` (kernel level only: y1 operands, coefficients and weights multiples of 1/2, 1/4; slopes 1/4: every value
up to y2 and out is exact in fp32, so extreme, arg, a1 and out are compared bit for bit, natural ties included) and `gauss`
(the probe is zeroed where the fp64 top-1 to top-2 gap, copies of the winner aside, is below TAU_GAP * rms(y2), and where
|bn2(y2)[j*]| is within TAU_KINK of the activation's kink; at most 1 % of the pairs may be zeroed).  The gauss inputs are
drawn again (at most 32 times) until no bn1(y1) lies within KINK1 of LeakyReLU_s1's kink in either mode, where the
derivative of a1 jumps inside fp32 rounding.

gamma2 has mixed signs everywhere.  The kernel-level cases also hold channels with gamma2 = 0.0 and -0.0 (max direction, zero
coefficient), where the contract still names the j of the extreme of y2.  The block-level cases do not: there every
activation of the channel equals act(beta2), the composed form's torch.max may route its gradient to any j, and dgamma2 of
that channel depends on the j chosen -- the two forms agree on the contract only where gamma2 != 0."""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

TINY = 1e-30
FACTOR, FLOOR = 8.0, 1e-7
TAU_GAP, TAU_KINK, KINK1 = 1e-4, 1e-4, 2e-6
MAX_ZEROED = 0.01
DOMINANT = 16.0
EPS, MOMENTUM = 1e-5, 0.1
C1 = 64
HUB = 1

SHAPES = {                       # (B, N, k, Co)
    'straddle': (2, 64, 20, 64),        # segments straddle 32-row tiles
    'tile': (1, 96, 32, 128),           # a segment is exactly one tile
    'multi': (2, 50, 5, 64),            # several segments per tile, partial last workgroup
    'k2': (1, 33, 2, 128),              # smallest k, odd N
    'oddk': (3, 40, 31, 64),            # odd k
}
MODES = ('train', 'eval')
GRAD_NAMES = ('x', 'W1', 'b1', 'gamma1', 'beta1', 'W2', 'b2', 'gamma2', 'beta2')


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def err(x, ref):
    ref = ref.double()
    if ref.numel() == 0:
        return 0.0
    return float((x.detach().double().cpu() - ref).abs().max() / max(float(ref.abs().max()), TINY))


def within(ek, e32, factor=FACTOR):
    return ek <= factor * e32 + FLOOR


def act(t, slope):
    return torch.where(t > 0, t, slope * t)


def lists(B, N, k, g):
    """idx [B,N,k] long: random with repeats, HUB at j1 and j2 of every list, point N - 1 in none -> (idx, j1 [N], j2)."""
    idx = torch.randint(0, N - 1, (B, N, k), generator=g)         # N - 1 is never drawn
    i = torch.arange(N)
    j1 = (i + 1) % (k - 1)
    idx[:, i, j1] = HUB
    idx[:, :, k - 1] = HUB
    return idx, j1, k - 1


def _bn(y, gamma, beta, rm, rv, train):
    """oracle.ref_cpu's BatchNorm on [B,C,...] -> (bn(y), running mean, running var); the buffers are copies."""
    p = {'weight': gamma, 'bias': beta, 'running_mean': rm.clone(), 'running_var': rv.clone()}
    return O._bn(p, '', y, train), p['running_mean'], p['running_var']


# ----------------------------------------------------------------------------- the block
def route(y2, gamma2, idx):
    """y2 [B,Co,N,k] -> (j* [B,Co,N] long, zext, gap to the best edge that is no copy of the winner, rms(y2))."""
    with torch.no_grad():
        B, Co, N, k = y2.shape
        up = (gamma2 >= 0).view(1, Co, 1, 1)
        f = torch.where(up, y2, -y2)
        top = f.max(dim=3).values
        ar = torch.arange(k).view(1, 1, 1, k)
        n = torch.where(f == top.unsqueeze(3), ar, k).min(dim=3).values
        nbr = idx.unsqueeze(1).expand(B, Co, N, k)
        same = nbr == nbr.gather(3, n.unsqueeze(3))
        second = f.masked_fill(same, -math.inf).max(dim=3).values
        zext = torch.where(up.squeeze(3), top, -top)
        return n, zext, top - second, float(y2.double().pow(2).mean().sqrt())


def block_tail(y1, p, idx, train, nstar=None):
    """From y1 [B,64,N,k] on -> dict(out [B,Co,N], a1, y2, nstar, zext, gap, rms, pre, running buffers)."""
    Co = p['W2'].shape[0]
    t1, rm1, rv1 = _bn(y1, p['gamma1'], p['beta1'], p['mean1'], p['var1'], train)
    a1 = act(t1, p['slope1'])
    y2 = F.conv2d(a1, p['W2'].view(Co, C1, 1, 1), p['b2'])
    n, zext, gap, rms = route(y2.detach(), p['gamma2'].detach(), idx)
    t2, rm2, rv2 = _bn(y2, p['gamma2'], p['beta2'], p['mean2'], p['var2'], train)
    pre = t2.gather(3, (n if nstar is None else nstar).unsqueeze(3)).squeeze(3)          # the explicit gather
    return {'out': act(pre, p['slope2']), 'pre': pre, 't1': t1, 'a1': a1, 'y2': y2, 'nstar': n, 'zext': zext, 'gap': gap,
            'rms': rms, 'mean1': rm1, 'var1': rv1, 'mean2': rm2, 'var2': rv2}


def block(x, p, idx, train, nstar=None):
    """x [B,C,N] -> block_tail's dict, y1 from oracle.ref_cpu.graph_feature and the first 1x1 convolution."""
    k = idx.shape[2]
    e = O.graph_feature(x, k, idx)
    y1 = F.conv2d(e, p['W1'].view(C1, -1, 1, 1), p['b1'])
    r = block_tail(y1, p, idx, train, nstar)
    r['y1'] = y1
    return r


def naive_block(x, p, idx, train):
    """get_graph_feature -> Conv2d -> BatchNorm2d -> LeakyReLU, twice, -> max over k, with torch.nn modules."""
    k = idx.shape[2]
    Co, C2 = p['W2'].shape[0], p['W1'].shape[1]
    dt = x.dtype
    c1 = torch.nn.Conv2d(C2, C1, 1, bias=p['b1'] is not None).to(dt)
    c2 = torch.nn.Conv2d(C1, Co, 1, bias=p['b2'] is not None).to(dt)
    b1, b2 = torch.nn.BatchNorm2d(C1, eps=EPS, momentum=MOMENTUM).to(dt), torch.nn.BatchNorm2d(Co, eps=EPS, momentum=MOMENTUM).to(dt)
    with torch.no_grad():
        c1.weight.copy_(p['W1'].view(C1, C2, 1, 1)), c2.weight.copy_(p['W2'].view(Co, C1, 1, 1))
        if p['b1'] is not None:
            c1.bias.copy_(p['b1'])
        if p['b2'] is not None:
            c2.bias.copy_(p['b2'])
        for bn, i in ((b1, '1'), (b2, '2')):
            bn.weight.copy_(p['gamma' + i]), bn.bias.copy_(p['beta' + i])
            bn.running_mean.copy_(p['mean' + i]), bn.running_var.copy_(p['var' + i])
    net = torch.nn.Sequential(c1, b1, torch.nn.LeakyReLU(p['slope1']), c2, b2, torch.nn.LeakyReLU(p['slope2'])).train(train)
    out = net(O.graph_feature(x, k, idx)).max(dim=-1)[0]
    return out, b1, b2


def _params(Co, g, family='gauss'):
    bias = Co == 128                      # the T-Net block (6 -> 64 -> 128, ReLU, biases) and the network's (LeakyReLU(0.2), none)
    s = 0.0 if bias else 0.2
    g1 = torch.randn(C1, generator=g)
    p = {'W1': torch.randn(C1, 6, generator=g) / 6 ** 0.5, 'b1': torch.randn(C1, generator=g) * 0.1 if bias else None,
         'gamma1': torch.where(g1 >= 0, g1.clamp_min(0.25), g1.clamp_max(-0.25)), 'beta1': torch.randn(C1, generator=g) * 0.2,
         'mean1': torch.linspace(-0.1, 0.3, C1), 'var1': torch.linspace(0.6, 1.4, C1),
         'W2': torch.randn(Co, C1, generator=g) / C1 ** 0.5, 'b2': torch.randn(Co, generator=g) * 0.1 if bias else None,
         'gamma2': torch.randn(Co, generator=g), 'beta2': torch.randn(Co, generator=g) * 0.2,
         'mean2': torch.linspace(-0.2, 0.2, Co), 'var2': torch.linspace(0.5, 1.5, Co), 'slope1': s, 'slope2': s}
    return p


def _cast(p, dtype, grad=False):
    out = {}
    for k_, v in p.items():
        if torch.is_tensor(v):
            v = v.detach().to(dtype).clone()
            if grad and k_ in GRAD_NAMES:
                v.requires_grad_(True)
        out[k_] = v
    return out


@functools.lru_cache(maxsize=None)
def block_case(name):
    """One ops.edgeconv2 case (gauss): x [B,3,N], idx, the parameters, the probes of both modes."""
    B, N, k, Co = SHAPES[name]
    for attempt in range(32):
        g = gen('edge2', name, attempt)
        x = torch.randn(B, 3, N, generator=g)
        x[:, :, HUB] = DOMINANT * x[:, :, HUB + 1]
        idx, j1, j2 = lists(B, N, k, g)
        p = _params(Co, g)
        gout = torch.randn(B, Co, N, generator=g)
        r = {m: block(x.double(), _cast(p, torch.float64), idx, m == 'train') for m in MODES}
        if all(float(r[m]['t1'].abs().min()) >= KINK1 for m in MODES):
            break
    else:
        raise AssertionError('could not draw %s off the kink of the first activation' % name)
    c = {'name': name, 'B': B, 'N': N, 'k': k, 'Co': Co, 'x': x, 'idx': idx, 'j1': j1, 'j2': j2, 'p': p, 'attempt': attempt}
    for m in MODES:
        t = r[m]['pre']
        bad = t.abs() < TAU_KINK * max(1.0, float(t.pow(2).mean().sqrt()))
        bad |= r[m]['gap'] < TAU_GAP * r[m]['rms']
        c['gout_' + m] = torch.where(bad, torch.zeros_like(gout), gout)
        c['zeroed_' + m] = float(bad.double().mean())
    return c


@functools.lru_cache(maxsize=None)
def block_reference(name, mode, dtype):
    """The block restatement of a case in 'float64' / 'float32' with the gradients of its probe; shared, read-only."""
    c = block_case(name)
    dt = getattr(torch, dtype)
    p = _cast(c['p'], dt, grad=True)
    x = c['x'].to(dt).clone().requires_grad_(True)
    r = block(x, p, c['idx'], mode == 'train')
    leaves = {'x': x, **{n: p[n] for n in GRAD_NAMES[1:] if p[n] is not None}}
    grads = torch.autograd.grad(r['out'], list(leaves.values()), c['gout_' + mode].to(dt), allow_unused=True)
    res = {k_: (v.detach() if torch.is_tensor(v) else v) for k_, v in r.items()}
    for n, gr in zip(leaves, grads):
        res['d' + n] = torch.zeros_like(leaves[n]) if gr is None else gr
    return res


# ----------------------------------------------------------------------------- the kernels alone (C ABI)
@functools.lru_cache(maxsize=None)
def kernel_case(name, family):
    """Inputs of sug_edge_expand_fwd / sug_edgemlp_max_layer_fwd_xf / sug_edge_expand_bwd called directly: pq [B,N,128], idx,
    coef1 / coef2 (scale | shift rows given, as in eval mode), W2, b2, gamma2, the slopes, dy1."""
    B, N, k, Co = SHAPES[name]
    g = gen('edge2-kernel', name, family)
    idx, j1, j2 = lists(B, N, k, g)
    if family == 'grid':
        half = lambda *s: torch.randint(-2, 3, s, generator=g).float() / 2
        pq = half(B, N, 2 * C1)
        pq[:, HUB, :C1] = DOMINANT * pq[:, HUB + 1, :C1]
        sc1 = half(C1) + 0.25                                                      # nonzero, mixed signs
        sh1 = torch.randint(-4, 5, (C1,), generator=g).float() / 4
        W2, b2 = half(Co, C1), torch.randint(-4, 5, (Co,), generator=g).float() / 4
        sc2 = torch.randint(-2, 3, (Co,), generator=g).float() / 2
        sh2 = torch.randint(-4, 5, (Co,), generator=g).float() / 4
        slope1 = slope2 = 0.25
    else:
        pq = torch.randn(B, N, 2 * C1, generator=g)
        pq[:, HUB, :C1] = DOMINANT * pq[:, HUB + 1, :C1]
        sc1, sh1 = torch.randn(C1, generator=g), torch.randn(C1, generator=g) * 0.2
        W2, b2 = torch.randn(Co, C1, generator=g) / C1 ** 0.5, torch.randn(Co, generator=g) * 0.1
        sc2, sh2 = torch.randn(Co, generator=g), torch.randn(Co, generator=g) * 0.2
        slope1 = slope2 = 0.2
    gamma2 = sc2.clone()                                   # the sign the kernel routes by = the sign of the scale it applies
    gamma2[3], gamma2[Co - 2], gamma2[5] = 0.0, 0.0, -0.0
    sc2 = torch.where(gamma2 == 0, torch.zeros(Co), sc2)
    if Co == 64:
        b2 = None
    return {'B': B, 'N': N, 'k': k, 'Co': Co, 'pq': pq, 'idx': idx, 'j1': j1, 'j2': j2, 'sc1': sc1, 'sh1': sh1, 'W2': W2,
            'b2': b2, 'gamma2': gamma2, 'sc2': sc2, 'sh2': sh2, 'slope1': slope1, 'slope2': slope2,
            'dy1': torch.randn(B, N, k, C1, generator=g)}


def kernel_reference(c, dtype):
    """y1 = P[idx] + Q, a1 = act1(sc1 y1 + sh1), y2 = a1.W2^T + b2, the routing, out = act2(sc2 zext + sh2); dpq of dy1."""
    B, N, k, Co = c['B'], c['N'], c['k'], c['Co']
    pq = c['pq'].to(dtype)
    P, Q = pq[:, :, :C1], pq[:, :, C1:]
    flat = (c['idx'] + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    y1 = P.reshape(B * N, C1)[flat].view(B, N, k, C1) + Q.unsqueeze(2)
    a1 = act(y1 * c['sc1'].to(dtype) + c['sh1'].to(dtype), c['slope1'])
    y2 = a1 @ c['W2'].to(dtype).t()
    if c['b2'] is not None:
        y2 = y2 + c['b2'].to(dtype)
    n, zext, gap, rms = route(y2.permute(0, 3, 1, 2), c['gamma2'], c['idx'])             # [B,Co,N]
    out = act(zext * c['sc2'].to(dtype).view(1, Co, 1) + c['sh2'].to(dtype).view(1, Co, 1), c['slope2'])
    dy = c['dy1'].to(dtype)
    dP = torch.zeros(B * N, C1, dtype=dtype).index_add_(0, flat, dy.reshape(-1, C1)).view(B, N, C1)
    return {'y1': y1, 'a1': a1, 'y2': y2, 'nstar': n.permute(0, 2, 1), 'zext': zext.permute(0, 2, 1), 'gap': gap.permute(0, 2, 1),
            'rms': rms, 'out': out.permute(0, 2, 1), 'dpq': torch.cat((dP, dy.sum(dim=2)), dim=2)}


# ----------------------------------------------------------------------------- the network
MODEL = dict(B=2, N=128, k=20, emb_dims=256, num_part=50, num_category=16)
MODEL_SEED = 11


PART_COUNT = [4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3]            # ShapeNet-Part: 16 categories, 50 parts
PART_FIRST = [sum(PART_COUNT[:i]) for i in range(len(PART_COUNT))]


def model_inputs(seed=MODEL_SEED, ignore=True):
    """(points [B,3,N], category [B] distinct, label [B,N] inside each category's part range; ignore: seven points of
    cloud 0 carry the ignore index)."""
    m = MODEL
    g = torch.Generator().manual_seed(seed)
    pts = O.synth_clouds(m['B'], m['N'], g).squeeze(-1).contiguous()                     # [B,3,N]
    cat = (torch.arange(m['B']) * 5 + seed) % m['num_category']                         # distinct categories
    lab = torch.stack([PART_FIRST[c] + torch.randint(0, PART_COUNT[c], (m['N'],), generator=g) for c in cat.tolist()])
    if ignore:
        lab[0, :7] = -100
    return pts, cat, lab


def build_model(cls, dropout=0.0, input_transform=True, seed=5):
    """DGCNNPartSeg at the test's size with every parameter and buffer drawn (BatchNorm weights of mixed sign in the
    EdgeConv blocks; fc3 of the transform small but not zero, so that the transform is no identity)."""
    m = MODEL
    torch.manual_seed(seed)
    net = cls(num_part=m['num_part'], num_category=m['num_category'], k=m['k'], emb_dims=m['emb_dims'], dropout=dropout,
              input_transform=input_transform)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, t in net.state_dict().items():
            if n.endswith('num_batches_tracked') or (n.startswith('bn') and n[2:3].isdigit()):
                continue                                       # bnK aliases convK.1
            if n.endswith('running_var'):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif n.endswith('running_mean'):
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
            elif n.startswith('transform_net.fc3'):
                t.copy_(torch.randn(t.shape, generator=g) * 0.05)
            elif t.dim() == 1 and n.endswith('weight'):        # BatchNorm / LayerNorm scale
                w = torch.randn(t.shape, generator=g) * 0.5 + 1.0
                if n.split('.')[0] in ('conv1', 'conv2', 'conv3', 'conv4', 'conv5'):
                    w[::7] = -w[::7]
                t.copy_(w)
            elif t.dim() == 1:
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
    return net


# relative to the channel's rms.  The candidates of a max over k are 64-term products: sqrt(64) * 6e-8 = 5e-7 each, 1e-6 for
# their difference (at 2e-7 a routing flip in block 2 was seen on the device: conv4's weight gradient off by 1.5e-3)
EDGE_MARGIN, ROWS_MARGIN, GAP_MARGIN = 5e-7, 2e-6, 1e-6


def _seq(sd, pre, x, train, dims, slope=0.2, track=None):
    """Conv -> BatchNorm -> LeakyReLU(slope) of the three modules under `pre` on [B,C,N(,k)] (dims = 1 or 2).
    track: a list that receives (margin, the smallest |BatchNorm output|), the distance of the layer to its activation's kink."""
    w, b = sd[pre + '.0.weight'], sd.get(pre + '.0.bias')
    y = F.conv2d(x, w, b) if dims == 2 else F.conv1d(x, w, b)
    p = {'weight': sd[pre + '.1.weight'], 'bias': sd[pre + '.1.bias'], 'running_mean': sd[pre + '.1.running_mean'],
         'running_var': sd[pre + '.1.running_var']}
    t = O._bn(p, '', y, train)
    if track is not None:
        track.append((EDGE_MARGIN if t.dim() == 4 and t.shape[-1] > 1 else ROWS_MARGIN, float((t.detach().abs() / _chan_rms(t)).min())))
    return F.leaky_relu(t, slope)


def _chan_rms(t):
    """rms per channel (dimension 1) of [B,C,...], broadcastable: in eval mode the channels are not normalised."""
    d = t.detach()
    return d.pow(2).mean(dim=[i for i in range(d.dim()) if i != 1], keepdim=True).sqrt().clamp_min(TINY)


def _max(t, track=None):
    """max over the last dimension; track receives (margin, the smallest top-1 to top-2 gap).  A maximum of exactly 0 is
    that of ReLU outputs which are all 0: a tie that carries no gradient whichever entry is picked."""
    if track is not None:
        top = t.detach().topk(2, dim=-1).values
        gap = ((top[..., 0] - top[..., 1]) / _chan_rms(t).squeeze(-1))[top[..., 0] != 0]
        track.append((GAP_MARGIN, float(gap.min()) if gap.numel() else math.inf))
    return t.max(dim=-1)[0]


def net_forward(sd, points, category, graphs, train, input_transform=True, k=20, drop=None, track=None):
    """DGCNNPartSeg on a flat state dict `sd` (the running buffers are updated in place), channels-first as the authors
    write it, the input transform from the layers of oracle.ref_cpu.transform_net in its DGCNN form (max over k behind
    conv2d2); graphs: four [B,N,k] long lists, or None to compute each with oracle.ref_cpu.knn_idx.
    -> (logits [B,N,num_part], global feature [B,emb], the lists used)."""
    B, _, N = points.shape
    used = [None] * 4
    S = lambda pre, x, dims, slope=0.2: _seq(sd, pre, x, train, dims, slope, track)

    def nb(f, i):
        used[i] = graphs[i] if graphs is not None and graphs[i] is not None else O.knn_idx(f, k)
        return used[i]

    x = points
    if input_transform:
        t = 'transform_net.'
        y = _max(S(t + 'conv2d2.conv', S(t + 'conv2d1.conv', O.graph_feature(x, k, nb(x, 0)), 2, 0.0), 2, 0.0), track)   # [B,128,N]
        y = _max(S(t + 'conv2d3.conv', y.unsqueeze(-1), 2, 0.0).squeeze(-1), track)                                       # [B,1024]
        y = O.fc_ln_act(sd, t + 'fc2.', O.fc_ln_act(sd, t + 'fc1.', y))
        T = (F.linear(y, sd[t + 'fc3.weight'], sd[t + 'fc3.bias']) + torch.eye(3, dtype=y.dtype).view(1, 9)).view(B, 3, 3)
        x = torch.bmm(x.transpose(1, 2), T).transpose(1, 2)
    x1 = _max(S('conv2', S('conv1', O.graph_feature(x, k, nb(x, 1)), 2), 2), track)
    x2 = _max(S('conv4', S('conv3', O.graph_feature(x1, k, nb(x1, 2)), 2), 2), track)
    x3 = _max(S('conv5', O.graph_feature(x2, k, nb(x2, 3)), 2), track)
    feats = torch.cat((x1, x2, x3), dim=1)                                               # [B,192,N]
    g = _max(S('conv6', feats, 1), track).unsqueeze(-1)
    nc = sd['conv7.0.weight'].shape[1]
    onehot = (category.view(B, 1) == torch.arange(nc).view(1, -1)).to(points.dtype).view(B, nc, 1)
    l = S('conv7', onehot, 1)
    h = torch.cat((torch.cat((g, l), dim=1).repeat(1, 1, N), feats), dim=1)               # [B,1280 (emb + 64 + 192),N]
    h = S('conv8', h, 1)
    h = S('conv9', h if drop is None else drop(h), 1)
    h = S('conv10', h if drop is None else drop(h), 1)
    logits = F.conv1d(h, sd['conv11.weight'])
    return logits.transpose(1, 2), g.squeeze(-1), used


def find_inputs(net_sd, train, input_transform=True, max_draws=2000):
    """The first input seed MODEL_SEED + 1000 d, d = 0, 1, .., whose fp64 forward keeps every BatchNorm output of an activated
    layer at least EDGE_MARGIN (k-expanded layers) / ROWS_MARGIN (per-point layers) times the channel's rms away from 0,
    and every max over k / over N a top-1 to top-2 gap of at least GAP_MARGIN times the channel's rms -> (seed, the
    forward's own neighbour lists, d).

    Why: LeakyReLU's derivative jumps at 0 and the arg of a max jumps at a tie.  An element that the device places on the
    other side (its fp32 error of these normalised O(1) values is some sqrt(K) * 6e-8: 5e-7 behind the 6 .. 128-term
    products of the edge layers, 2e-6 behind the 192 .. 1280-term ones of the per-point layers) changes ONE summand of a
    BatchNorm-bias gradient by 0.8 of its size -- measured: 1e-2 of such a gradient at 256 rows, and 1e-3 of everything
    upstream -- which is a property of the input, not an error of either side.  The candidates of a max are held GAP_MARGIN
    apart.  With build_model's parameters draw 10 (train), 0 (train, no transform) and 27 (eval) pass, 30 ms a draw; the
    search is a function of the parameters and the mode only."""
    sd64 = {n: t.detach().double() if t.is_floating_point() else t for n, t in net_sd.items()}
    for d in range(max_draws):
        seed = MODEL_SEED + 1000 * d
        pts, cat, _ = model_inputs(seed)
        sd = {n: t.clone() for n, t in sd64.items()}
        track = []
        with torch.no_grad():
            used = net_forward(sd, pts.double(), cat, None, train, input_transform, MODEL['k'], track=track)[2]
        if all(v >= m for m, v in track):
            return seed, used, d
    raise AssertionError('no input within %d draws keeps the margins' % max_draws)


def head_split(W8, g, l, feats):
    """conv8's product in the split form of the model: per-cloud columns once per cloud + per-point columns."""
    ng = g.shape[1] + l.shape[1]
    cloud = torch.cat((g, l), dim=1) @ W8[:, :ng].t()                                   # [B,256]
    return feats @ W8[:, ng:].t() + cloud.unsqueeze(1)                                    # feats [B,N,192]


def head_concat(W8, g, l, feats):
    N = feats.shape[1]
    return torch.cat((torch.cat((g, l), dim=1).unsqueeze(1).expand(-1, N, -1), feats), dim=2) @ W8.t()


def run_reference(net_sd, dtype, train, input_transform=True, graphs=None, seed=MODEL_SEED):
    """The restated network with the per-point cross entropy (mean over the labelled points) -> logits, feat, loss, the
    parameter gradients by name, the updated buffers, the lists used."""
    pts, cat, lab = model_inputs(seed)
    sd = {n: t.detach().to(dtype).clone() if t.is_floating_point() else t.clone() for n, t in net_sd.items()}
    names = [n for n, t in sd.items() if t.is_floating_point() and 'running_' not in n
             and not (n.startswith('bn') and n[2:3].isdigit())]
    for n in names:
        sd[n].requires_grad_(True)
    logits, feat, used = net_forward(sd, pts.to(dtype), cat, graphs, train, input_transform, MODEL['k'])
    loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), lab.reshape(-1), ignore_index=-100)
    grads = torch.autograd.grad(loss, [sd[n] for n in names], allow_unused=True)
    return {'logits': logits.detach(), 'feat': feat.detach(), 'loss': float(loss.detach()), 'names': names,
            'grads': {n: (torch.zeros_like(sd[n]) if g_ is None else g_) for n, g_ in zip(names, grads)},
            'buffers': {n: t.detach() for n, t in sd.items() if 'running_' in n and not n.startswith('bn')}, 'graphs': used}
