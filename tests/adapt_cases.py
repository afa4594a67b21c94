"""Plain fp64 restatements of the SA-node glue kernels of sug_amd/csrc/adapt.hip (node_offset, interp3_cat), the case
builders of tests/test_adapt_host.py and tests/test_gpu_adapt.py, and the child process that runs the unordered
node_offset backward forms (the switch SUG_NODE_OFFSET_UNORDERED is read once per process).

Every operation is written out in plain torch from the reference's model/model_utils.py:110-119 (adapt_layer_off) and
model/point_utils.py:156-162 (upsample_inter); inputs are upcast to `dtype` (fp64 for the reference, fp32 for the "same
formula in plain fp32" baseline of the error bound).  Gradients come from torch.autograd on these restatements, never
from a second hand-derived formula.  Nothing at module level imports sug_amd: the module is usable on the CPU.

The bound of the GPU tests, per output tensor:  err(x) = max|x - ref64| / max(max|ref64|, tiny)  and
err(kernel) <= 8 * err(fp32 torch) + 1e-7.  The factor covers tanhf / division differing from torch's by a few ulp and
another summation order over up to a few hundred colliding terms; a wrong term, a dropped duplicate or a mis-pipelined
node is an error of order 1 in this metric."""
import json
import os
import sys
import zlib

import torch

PATTERNS = ('random', 'few', 'padded', 'constant', 'sentinel')
TINY = 1e-30
FACTOR, FLOOR = 8.0, 1e-7


def gen(*key):
    """A generator seeded by the case's name (stable across processes, unlike hash())."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ----------------------------------------------------------------------------- restatements
def rows(t, idx):
    """t [B,N,C], idx [B,...] (long, in range) -> t[b, idx[b, ...], :]: a gather by index (its gradient is an index_add)."""
    B = t.shape[0]
    return t[torch.arange(B).view([B] + [1] * (idx.dim() - 1)), idx]


def node_offset_ref(proj, loc, fidx, gidx, dtype=torch.float64):
    """off[b,s] = (1/ns) sum_j valid_j tanh(proj[g_j] - proj[f]) (loc[g_j] - loc[f]),  nloc = loc[f] + off
    with valid_j = 0 <= g_j < N (a zero-hit row of the ball query holds N) and f = clamp(fidx, 0, N-1).
    proj, loc [B,N,3]; fidx [B,S]; gidx [B,S,ns] -> (off, nloc) [B,S,3] in `dtype`, differentiable in proj."""
    proj, loc = proj.to(dtype), loc.to(dtype)
    N, ns = proj.shape[1], gidx.shape[2]
    f = fidx.long().clamp(0, N - 1)
    g = gidx.long()
    valid = ((g >= 0) & (g < N)).to(dtype).unsqueeze(-1)
    gs = g.clamp(0, N - 1)
    lc = rows(loc, f)
    term = torch.tanh(rows(proj, gs) - rows(proj, f).unsqueeze(2)) * (rows(loc, gs) - lc.unsqueeze(2)) * valid
    off = term.sum(dim=2) / ns
    return off, lc + off


def interp3_cat_ref(fea, node, xyz, nloc, idx3, d3, dtype=torch.float64):
    """cat(fea, sum_t w_t node[idx3_t]),  w = (1 / where(d < 1e-10, 1e-10, d)) / sum.
    The VALUE of d is the d3 the caller passes in (the fp32 distances the kernel was given, so the weights carry no
    cancellation error of an expanded-form 3-NN); its GRADIENT is that of e = |xyz - nloc[idx3]|^2, through
    d = d3 + (e - e.detach()): upsample_inter's gradient to node and nloc, zero where clamped.
    fea [B,N,C1], node [B,S,C2], xyz [B,N,3], nloc [B,S,3], idx3 / d3 [B,N,3] -> [B,N,C1+C2] in `dtype`."""
    fea, node, xyz, nloc = (t.to(dtype) for t in (fea, node, xyz, nloc))
    i = idx3.long()
    e = ((xyz.unsqueeze(2) - rows(nloc, i)) ** 2).sum(-1)
    d = d3.to(dtype) + (e - e.detach())
    d = torch.where(d < 1e-10, torch.full_like(d, 1e-10), d)
    w = 1.0 / d
    w = w / w.sum(dim=-1, keepdim=True)
    return torch.cat([fea, (rows(node, i) * w.unsqueeze(-1)).sum(dim=2)], dim=-1)


def node_offset_all(c, dtype):
    """-> {'off', 'nloc', 'dproj/off', 'dproj/nloc', 'dproj/both'} of case c in `dtype` (autograd of node_offset_ref)."""
    p = c['proj'].to(dtype).clone().requires_grad_(True)
    off, nloc = node_offset_ref(p, c['loc'], c['fidx'], c['gidx'], dtype)
    go, gn = c['goff'].to(dtype), c['gnloc'].to(dtype)
    out = {'off': off.detach(), 'nloc': nloc.detach()}
    for name, outs, gs in (('off', [off], [go]), ('nloc', [nloc], [gn]), ('both', [off, nloc], [go, gn])):
        out['dproj/' + name] = torch.autograd.grad(outs, p, gs, retain_graph=True)[0]
    return out


def interp3_cat_all(c, idx3, d3, dtype):
    """-> {'out', 'dfea', 'dnode', 'dnloc'} of case c in `dtype` for the gradient c['g'] of out."""
    fea, node, nloc = (c[k].to(dtype).clone().requires_grad_(True) for k in ('fea', 'node', 'nloc'))
    out = interp3_cat_ref(fea, node, c['xyz'], nloc, idx3.cpu(), d3.cpu(), dtype)
    dfea, dnode, dnloc = torch.autograd.grad(out, (fea, node, nloc), c['g'].to(dtype))
    return {'out': out.detach(), 'dfea': dfea, 'dnode': dnode, 'dnloc': dnloc}


# ----------------------------------------------------------------------------- cases
def indices(pattern, B, N, S, ns, g):
    """-> (fidx [B,S], gidx [B,S,ns]) int32 of one of PATTERNS, straight from torch.randint."""
    fidx = torch.randint(0, N, (B, S), generator=g)
    gidx = torch.randint(0, N, (B, S, ns), generator=g)
    if pattern == 'random':
        pass
    elif pattern == 'few':               # every row (and every centre) drawn from 5 points of the cloud: worst collisions
        pool = torch.randint(0, N, (B, 5), generator=g)
        gidx = torch.gather(pool, 1, torch.randint(0, 5, (B, S * ns), generator=g)).view(B, S, ns)
        fidx = torch.gather(pool, 1, torch.randint(0, 5, (B, S), generator=g))
    elif pattern == 'padded':            # a random prefix, the rest a repeat of the first entry (the ball query's padding)
        count = torch.randint(1, ns + 1, (B, S, 1), generator=g)
        gidx = torch.where(torch.arange(ns).view(1, 1, ns) < count, gidx, gidx[:, :, :1])
    elif pattern == 'constant':          # all ns entries the same point; in every second row that point is the centre
        c = torch.randint(0, N, (B, S), generator=g)
        gidx = c.unsqueeze(-1).expand(B, S, ns).clone()
        fidx = torch.where(torch.arange(S).view(1, S) % 2 == 0, c, fidx)
    elif pattern == 'sentinel':
        # valid entries name the lower three quarters only, so some points are named by nobody; rows s % 4 == 0 are
        # entirely N (zero-hit), rows s % 4 == 1 have N and -1 scattered in; one centre is N and one is -1
        hi = max(1, N - N // 4)
        fidx = torch.randint(0, hi, (B, S), generator=g)
        gidx = torch.randint(0, hi, (B, S, ns), generator=g)
        s = torch.arange(S).view(1, S, 1)
        u = torch.rand(B, S, ns, generator=g)
        gidx = torch.where((s % 4 == 1) & (u < 0.3), torch.full_like(gidx, N), gidx)
        gidx = torch.where((s % 4 == 1) & (u > 0.8), torch.full_like(gidx, -1), gidx)
        gidx = torch.where(s % 4 == 0, torch.full_like(gidx, N), gidx)
        fidx[:, S - 1] = N
        fidx[:, S // 2] = -1
    else:
        raise ValueError(pattern)
    return fidx.to(torch.int32), gidx.to(torch.int32).contiguous()


def node_case(pattern, B, N, S, ns):
    """One node_offset case: proj, loc [B,N,3] fp32, fidx, gidx, and the gradients of off and of nloc."""
    g = gen('node', pattern, B, N, S, ns)
    c = {'proj': torch.randn(B, N, 3, generator=g), 'loc': torch.rand(B, N, 3, generator=g) * 2 - 1}
    c['fidx'], c['gidx'] = indices(pattern, B, N, S, ns, g)
    c['goff'] = torch.randn(B, S, 3, generator=g)
    c['gnloc'] = torch.randn(B, S, 3, generator=g)
    return c


def named_points(c):
    """[B,N] bool: the points a valid gidx entry or a (clamped) centre names -- every other row of dproj is exactly 0."""
    B, N, _ = c['proj'].shape
    g = c['gidx'].long().reshape(B, -1)
    ok = (g >= 0) & (g < N)
    m = torch.zeros(B, N + 1, dtype=torch.bool)
    m.scatter_(1, torch.where(ok, g, torch.full_like(g, N)), True)
    m = m[:, :N].clone()
    m.scatter_(1, c['fidx'].long().clamp(0, N - 1), True)
    return m


def empty_nodes(c):
    """[B,S] bool: the nodes whose gidx row holds no valid entry."""
    N = c['proj'].shape[1]
    g = c['gidx'].long()
    return ~((g >= 0) & (g < N)).any(dim=-1)


def interp_case(B, N, S, C1, C2, tag=''):
    """One interp3_cat case: fea [B,N,C1], node [B,S,C2], xyz [B,N,3], nloc [B,S,3], g [B,N,C1+C2], all fp32."""
    g = gen('interp', B, N, S, C1, C2, tag)
    return {'fea': torch.randn(B, N, C1, generator=g), 'node': torch.randn(B, S, C2, generator=g),
            'xyz': torch.rand(B, N, 3, generator=g) * 2 - 1, 'nloc': torch.rand(B, S, 3, generator=g) * 2 - 1,
            'g': torch.randn(B, N, C1 + C2, generator=g)}


# ----------------------------------------------------------------------------- error measure
def err(x, ref):
    ref = ref.double()
    if ref.numel() == 0:
        return 0.0
    return float((x.detach().double().cpu() - ref).abs().max() / max(float(ref.abs().max()), TINY))


def errors(got, ref64, ref32):
    """{name: (err(kernel), err(fp32 torch))} over the tensors of `got`."""
    return {k: (err(got[k], ref64[k]), err(ref32[k], ref64[k])) for k in got}


def within(ek, e32):
    return ek <= FACTOR * e32 + FLOOR


# ----------------------------------------------------------------------------- on the GPU
def run_node_offset(c):
    """ops.node_offset forward and the three backward forms (through off, through nloc, through both) of case c."""
    from sug_amd import ops
    proj = c['proj'].cuda().requires_grad_(True)
    loc, fidx, gidx = c['loc'].cuda(), c['fidx'].cuda(), c['gidx'].cuda()
    go, gn = c['goff'].cuda(), c['gnloc'].cuda()
    off, nloc = ops.node_offset(proj, loc, fidx, gidx)
    got = {'off': off.detach(), 'nloc': nloc.detach()}
    for name, outs, gs in (('off', [off], [go]), ('nloc', [nloc], [gn]), ('both', [off, nloc], [go, gn])):
        got['dproj/' + name] = torch.autograd.grad(outs, proj, gs, retain_graph=True)[0]
    return {k: v.cpu() for k, v in got.items()}


def measure_node_offset(c):
    """-> (outputs of the kernels on the CPU, {name: (err(kernel), err(fp32 torch))})."""
    got = run_node_offset(c)
    return got, errors(got, node_offset_all(c, torch.float64), node_offset_all(c, torch.float32))


UNORDERED_CASES = [('lds-atomic', 1024, 'padded'), ('lds-atomic', 1024, 'sentinel'),
                   ('global-atomic', 6000, 'padded'), ('global-atomic', 6000, 'sentinel')]


def unordered_main(path):
    """The child of test_node_offset_unordered_lds_atomic_and_global_atomic: runs UNORDERED_CASES in a process started
    with SUG_NODE_OFFSET_UNORDERED=1 and writes {case id: {'errors': {name: [err(kernel), err(fp32 torch)]},
    'unnamed_max': largest |dproj| over the rows nobody names, 'empty_max': largest |off| over the all-sentinel nodes}}."""
    assert os.environ.get('SUG_NODE_OFFSET_UNORDERED') == '1'
    res = {}
    for form, N, pattern in UNORDERED_CASES:
        c = node_case(pattern, 2, N, 64, 64)
        got, errs = measure_node_offset(c)
        un, em = ~named_points(c), empty_nodes(c)
        res['%s-N%d-%s' % (form, N, pattern)] = {
            'errors': {k: list(v) for k, v in errs.items()},
            'unnamed_max': max(float(got['dproj/' + k][un].abs().max()) if un.any() else 0.0 for k in ('off', 'nloc', 'both')),
            'empty_max': float(got['off'][em].abs().max()) if em.any() else 0.0}
    with open(path, 'w') as f:
        json.dump(res, f)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) == 3 and sys.argv[1] == '--unordered':
        unordered_main(sys.argv[2])
    else:
        sys.exit('usage: adapt_cases.py --unordered OUT.json')
