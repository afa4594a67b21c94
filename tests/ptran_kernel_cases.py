"""Plain fp64 restatements of the Point Transformer attention kernels (sug_ptran_*), and the case generators
of tests/test_ptran_kernels_host.py, tests/test_gpu_ptran_kernels.py and tests/test_gpu_ptran.py.

Every operation is written out in plain torch from the reference's model/Ptran_transformer.py:39-44; inputs are
upcast to `dtype` (fp64 for the reference, fp32 for the "same restatement in plain fp32" baseline of the error-ratio
bars).  Gradients come from torch.autograd on these restatements, never from a second hand-derived formula.
Nothing here imports sug_amd: the module is usable on the CPU."""
import math
import zlib

import numpy as np
import torch

D = 512
SCALE = 1.0 / math.sqrt(D)

# (B, n, k): smallest possible | B*n no multiple of a workgroup's 4 waves, p / n crosses clouds | full k |
# k % 4 != 0 (the j0 + t < k guards) | odd k below half | several workgroups, grid-stride column sums
SHAPES = [(1, 1, 1), (2, 5, 4), (3, 16, 16), (2, 37, 15), (2, 64, 7), (1, 300, 16)]
LIST_KINDS = ('knn', 'random', 'hub', 'padded')
REGIMES = ('uniform', 'peaked', 'saturated', 'equal_pos', 'equal_neg')      # (e), k = 1, is the shape (1, 1, 1)


def gen(*key):
    """A generator seeded by the case's name (stable across processes, unlike hash())."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ----------------------------------------------------------------------------- restatements
def gather(t, nbr):
    """t [B,n,C], nbr [B,n,k] -> [B,n,k,C]: row nbr[b,i,j] of cloud b."""
    B = t.shape[0]
    return t[torch.arange(B)[:, None, None], nbr.long()]


def pos1(xyz, nbr, w1, b1, dtype=torch.float64):
    """T0 = relu(W1 . (xyz_i - xyz_nbr) + b1)   (fc_delta[0] + ReLU, :39)"""
    xyz, w1, b1 = xyz.to(dtype), w1.to(dtype), b1.to(dtype)
    rel = xyz[:, :, None] - gather(xyz, nbr)
    return torch.relu(rel @ w1.t() + b1)


def qk(q, kf, delta, nbr, dtype=torch.float64):
    """U = q_i - K_nbr + delta   (input of fc_gamma, :41)"""
    q, kf, delta = q.to(dtype), kf.to(dtype), delta.to(dtype)
    return q[:, :, None] - gather(kf, nbr) + delta


def attn(logits, delta, vf, nbr, dtype=torch.float64, scale=SCALE):
    """mixed = sum_j softmax_j(L / sqrt(d)) * (V_nbr + delta)   (:42-44)
    -> (mixed [B,n,d], per-channel max of L / sqrt(d), sum of exp(L / sqrt(d) - max), weights [B,n,k,d])"""
    z = logits.to(dtype) * scale
    mx = z.max(dim=2)[0]
    e = torch.exp(z - mx[:, :, None])
    sm = e.sum(dim=2)
    a = e / sm[:, :, None]
    y = gather(vf.to(dtype), nbr) + delta.to(dtype)
    return (a * y).sum(dim=2), mx, sm, a


def relu_mask(G, T1, dtype=torch.float64):
    """sug_ptran_relu_bwd_db: G * [T1 > 0] and its column sums (the gradient of relu by autograd)."""
    t = T1.to(dtype).clone().requires_grad_(True)
    (m,) = torch.autograd.grad(torch.relu(t), t, G.to(dtype))
    return m, m.reshape(-1, m.shape[-1]).sum(0)


def attn_grads(g, logits, delta, vf, nbr, dtype=torch.float64):
    """autograd of attn: (dL, da = gradient of delta through v + delta, dV, column sums of dL)"""
    L, dl, v = (t.to(dtype).clone().requires_grad_(True) for t in (logits, delta, vf))
    mixed = attn(L, dl, v, nbr, dtype)[0]
    dL, da, dV = torch.autograd.grad(mixed, (L, dl, v), g.to(dtype))
    return dL, da, dV, dL.reshape(-1, D).sum(0)


def qk_grads(dU, da, nbr, B, n, dtype=torch.float64):
    """autograd of qk with delta's second gradient `da` added: (dq, dK, d delta = dU + da, column sums of d delta)"""
    k = nbr.shape[2]
    q, kf = (torch.zeros(B, n, D, dtype=dtype, requires_grad=True) for _ in range(2))
    delta = torch.zeros(B, n, k, D, dtype=dtype, requires_grad=True)
    loss = (qk(q, kf, delta, nbr, dtype) * dU.to(dtype)).sum() + (delta * da.to(dtype)).sum()
    dq, dK, dd = torch.autograd.grad(loss, (q, kf, delta))
    return dq, dK, dd, dd.reshape(-1, D).sum(0)


def pos1_grads(g, xyz, nbr, w1, b1, dtype=torch.float64):
    """autograd of pos1: (dW1 [512,3], db1 [512])"""
    w, b = (t.to(dtype).clone().requires_grad_(True) for t in (w1, b1))
    return torch.autograd.grad(pos1(xyz, nbr, w, b, dtype), (w, b), g.to(dtype))


def block_forward(p, xyz, feat, nbr, dtype=torch.float64, keep_graph=False):
    """TransformerBlock.forward composed of the restatements in order, on given neighbour lists.  p: the block's
    state_dict (any dtype; keep_graph: leaves of `dtype` that autograd should reach) -> (out, every intermediate)."""
    P = p if keep_graph else {k: v.detach().to(dtype) for k, v in p.items()}

    def lin(name, t):
        y = t @ P[name + '.weight'].t()
        return y + P[name + '.bias'] if name + '.bias' in P else y
    xyz, feat = xyz.to(dtype), feat.to(dtype)
    x = lin('fc1', feat)
    q, kf, vf = lin('w_qs', x), lin('w_ks', x), lin('w_vs', x)
    T0 = pos1(xyz, nbr, P['fc_delta.0.weight'], P['fc_delta.0.bias'], dtype)
    delta = lin('fc_delta.2', T0)
    U = qk(q, kf, delta, nbr, dtype)
    T1 = torch.relu(lin('fc_gamma.0', U))
    Lg = lin('fc_gamma.2', T1)
    mixed, mx, sm, a = attn(Lg, delta, vf, nbr, dtype)
    return lin('fc2', mixed) + feat, {'q': q, 'kf': kf, 'vf': vf, 'T0': T0, 'delta': delta, 'U': U, 'T1': T1, 'L': Lg,
                                      'mixed': mixed, 'mx': mx, 'sm': sm, 'attn': a}


def block_grads(blk_state, xyz, feat, nbr, probe, dtype=torch.float64):
    """(block(feat) * probe).sum() by autograd on block_forward -> (out, d feat, {dq, dK, dV}, {parameter: gradient})"""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in blk_state.items()}
    f = feat.detach().to(dtype).clone().requires_grad_(True)
    out, mid = block_forward(P, xyz, f, nbr, dtype, keep_graph=True)
    names = sorted(P)
    wrt = [f, mid['q'], mid['kf'], mid['vf'], mid['L']] + [P[k] for k in names]
    grads = torch.autograd.grad(out, wrt, probe.to(dtype), allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, wrt)]
    return out.detach(), grads[0], {'dq': grads[1], 'dK': grads[2], 'dV': grads[3], 'dL': grads[4]}, dict(zip(names, grads[5:]))


def attention_grads(state, xyz, nbr, q, kf, vf, g, dtype=torch.float64):
    """ops.ptran_attention's part of the block, from given q / K / V: (mixed, {dq, dK, dV}, {parameter: gradient}) of
    (mixed * g).sum() for the fc_delta / fc_gamma parameters in `state`."""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    q, kf, vf = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, kf, vf))

    def lin(name, t):
        return t @ P[name + '.weight'].t() + P[name + '.bias']
    delta = lin('fc_delta.2', pos1(xyz, nbr, P['fc_delta.0.weight'], P['fc_delta.0.bias'], dtype))
    Lg = lin('fc_gamma.2', torch.relu(lin('fc_gamma.0', qk(q, kf, delta, nbr, dtype))))
    mixed = attn(Lg, delta, vf, nbr, dtype)[0]
    names = sorted(P)
    grads = torch.autograd.grad(mixed, [q, kf, vf, Lg] + [P[k] for k in names], g.to(dtype))
    return mixed.detach(), {'dq': grads[0], 'dK': grads[1], 'dV': grads[2], 'dL': grads[3]}, dict(zip(names, grads[4:]))


# ----------------------------------------------------------------------------- neighbour lists
def true_knn(xyz, k, self_first=True):
    """Exact kNN of xyz [B,n,3] (fp64 squared distances, ties by index); self_first puts point i first in its list."""
    x = xyz.double()
    d = ((x[:, :, None] - x[:, None]) ** 2).sum(-1)
    if self_first:
        n = x.shape[1]
        d[:, torch.arange(n), torch.arange(n)] = -1.0
    return torch.from_numpy(np.argsort(d.numpy(), axis=-1, kind='stable')[:, :, :k].copy()).to(torch.int32)


def neighbours(kind, B, n, k):
    """-> (xyz [B,n,3] fp32, nbr [B,n,k] int32) of one of LIST_KINDS."""
    g = gen('nbr', kind, B, n, k)
    xyz = torch.rand(B, n, 3, generator=g)
    if kind == 'knn':                # (i) true kNN, self first
        assert k <= n
        return xyz, true_knn(xyz, k)
    if kind == 'random':             # (ii) uniformly random, repeats inside a row
        return xyz, torch.randint(0, n, (B, n, k), generator=g).to(torch.int32)
    if kind == 'hub':                # (iii) column 0 is point 0; the rest from the first half: the second half are orphans
        nbr = torch.randint(0, max(1, n // 2), (B, n, k), generator=g).to(torch.int32)
        nbr[:, :, 0] = 0
        return xyz, nbr
    if kind == 'padded':             # (iv) the last third are exact copies of point 0; plain kNN, ties by index
        assert k <= n
        if n // 3:
            xyz[:, n - n // 3:] = xyz[:, :1]
        return xyz, true_knn(xyz, k, self_first=False)
    raise ValueError(kind)


def orphans(n):
    """The points of a 'hub' list that no list names."""
    return list(range(max(1, n // 2), n))


def reverse_lists(nbr):
    """numpy construction of the reverse lists: off [B,n+1], ent [B,n*k] (entry e = i*k + j names nbr[b,i,j]; ascending)."""
    B, n, k = nbr.shape
    a = nbr.numpy().reshape(B, n * k)
    off = np.zeros((B, n + 1), np.int32)
    ent = np.zeros((B, n * k), np.int32)
    for b in range(B):
        order = np.argsort(a[b], kind='stable')          # by destination, entries ascending within one
        ent[b] = order
        off[b, 1:] = np.cumsum(np.bincount(a[b], minlength=n))
    return off, ent


# ----------------------------------------------------------------------------- logits
def logits(regime, B, n, k):
    """-> L [B,n,k,512] fp32, every value exactly representable in fp16 where the regime needs it (c, d)."""
    g = gen('logits', regime, B, n, k)
    if regime == 'uniform':          # (a) today's regime: |L / sqrt(d)| <= ~0.05
        return 0.3 * torch.randn(B, n, k, D, generator=g)
    if regime == 'peaked':           # (b) L / sqrt(d) = 5 * randn: about +-10 over 16 neighbours
        return (5.0 / SCALE) * torch.randn(B, n, k, D, generator=g)
    if regime == 'saturated':        # (c) one neighbour per (point, channel) above the rest by >= 2e4; multiples of 16
        L = 16.0 * torch.randint(-2, 3, (B, n, k, D), generator=g).float()
        sel = torch.randint(0, k, (B, n, 1, D), generator=g)
        L.scatter_(2, sel, 20032.0)
        return L
    if regime in ('equal_pos', 'equal_neg'):     # (d) all k logits equal and large, no noise
        return torch.full((B, n, k, D), 3e4 if regime == 'equal_pos' else -3e4)
    raise ValueError(regime)


def selected(L):
    """The index of the largest logit per (point, channel): [B,n,1,512]."""
    return L.argmax(dim=2, keepdim=True)


def attn_inputs(B, n, k, lo=torch.float32):
    """delta [B,n,k,512] (rounded to `lo`), V [B,n,512], g [B,n,512].
    fp32: g = randn, |V + delta| up to ~10.  fp16: g = 0.5 * randn and |V + delta| <= ~1, because of the winning neighbour
    of a peaked softmax: there a ~ 1 and y ~ mixed, so dL = a (g y - g mixed) / sqrt(d) is the difference of two fp32 products
    of size |g y| and carries about 5 roundings of them, 5 * 2^-24 |g y| / sqrt(512) = 0.22 * 2^-24 |g y|, however small dL
    itself is.  The fp16 bar is an fp16 ulp around the fp64 result: after the output rounding (2^-11 |ref| + 2^-25) it has
    2^-25 left for fp32 arithmetic, which holds for |g y| <= 2.3."""
    g = gen('attn_in', B, n, k)
    amp, gamp = (1.0, 1.0) if lo == torch.float32 else (0.15, 0.5)
    delta = (amp * torch.randn(B, n, k, D, generator=g)).to(lo)
    vf = 2.0 * amp * torch.randn(B, n, D, generator=g) if lo == torch.float32 else amp * torch.randn(B, n, D, generator=g)
    gr = gamp * torch.randn(B, n, D, generator=g)
    return delta, vf, gr


def qk_inputs(B, n, k, lo=torch.float32):
    """q, K [B,n,512] and delta [B,n,k,512] (rounded to `lo`).  q and K are 0.25 * randn so that |q - K| < 2: the fp32
    rounding of that difference (at most 2^-24 below 2) then stays inside the absolute term of the fp16 bar where
    q - K and delta cancel; the bar is an fp16 ulp around the fp64 result and has no room for fp32 cancellation error."""
    g = gen('qk_in', B, n, k)
    q = 0.25 * torch.randn(B, n, D, generator=g)
    kf = 0.25 * torch.randn(B, n, D, generator=g)
    delta = torch.randn(B, n, k, D, generator=g).to(lo)
    return q, kf, delta


def pos1_inputs(B, n, dyadic):
    """W1 [512,3], b1 [512].  dyadic: multiples of 2^-8 (use with dyadic_xyz): W1 . rel + b1 is then exact in fp32
    and in fp64, so the ReLU mask of the backward is the same in every precision (a pre-activation within rounding of 0
    would otherwise flip a whole gradient contribution and say nothing about the kernel)."""
    g = gen('pos1_in', B, n, dyadic)
    w1 = torch.randn(D, 3, generator=g)
    b1 = 0.5 * torch.randn(D, generator=g)
    if dyadic:
        w1, b1 = torch.round(w1 * 256) / 256, torch.round(b1 * 256) / 256
    return w1, b1


def dyadic_xyz(xyz):
    """Coordinates rounded to multiples of 2^-6 (copies stay copies; the neighbour lists are kept as given)."""
    return torch.round(xyz * 64) / 64


# ----------------------------------------------------------------------------- error measures
def rel_l2(got, ref):
    ref = ref.double()
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def within_fp16_ulp(got, ref):
    """|got - ref| <= 2^-10 |ref| + 2^-24: one fp16 unit in the last place around the fp64 result plus the
    subnormal spacing.  -> (ok, worst excess ratio)"""
    ref = ref.double()
    err = (got.double() - ref).abs()
    bar = ref.abs() * 2.0 ** -10 + 2.0 ** -24
    return bool((err <= bar).all()), float((err / bar).max())
