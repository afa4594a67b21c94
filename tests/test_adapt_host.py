"""CPU: the fp64 restatements of tests/adapt_cases.py are right -- they equal the oracle's adapt_layer_off / upsample_inter
in fp64 (values and gradients) and agree with torch.autograd.gradcheck -- and the case builders produce the index
patterns the GPU tests rely on."""
import pytest
import torch
import torch.nn.functional as F

import adapt_cases as C
from oracle import ref_cpu as O


def _adapt_params(seed):
    shapes = {'a.pred_offset.0.weight': (3, 64, 1, 1), 'a.residual.conv.0.weight': (64, 64, 1, 1),
              'a.residual.conv.0.bias': (64,), 'a.residual.conv.1.weight': (64,), 'a.residual.conv.1.bias': (64,),
              'a.residual.conv.1.running_mean': (64,), 'a.residual.conv.1.running_var': (64,)}
    p = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in O.fill_params(shapes, seed).items()}
    return O.as_params(p)


def test_node_offset_ref_equals_the_oracle_in_fp64():
    g = torch.Generator().manual_seed(31)
    B, N, S = 2, 300, 64
    loc = O.synth_clouds(B, N, g).squeeze(-1).double()                # [B,3,N]
    fea = torch.randn(B, 64, N, 1, generator=g).double().requires_grad_(True)
    start = torch.randint(0, N, (B,), generator=g)
    p = _adapt_params(5)
    _, _, off_o = O.adapt_layer_off(p, 'a.', fea, loc, True, start)   # [B,3,S]
    fidx = O.fps_cf(loc, S, start)
    gidx = O.ball_query_cf(0.3, 64, loc, O.gather_cf(loc, fidx))
    assert int((gidx == gidx[:, :, :1]).sum(-1).max()) > 1, 'the ball query pads here: duplicates inside a row'
    f2 = fea.detach().clone().requires_grad_(True)
    proj = f2.squeeze(-1).transpose(1, 2) @ p['a.pred_offset.0.weight'].detach().view(3, 64).t()
    off, nloc = C.node_offset_ref(proj, loc.transpose(1, 2), fidx, gidx)
    assert off.dtype == torch.float64
    torch.testing.assert_close(off, off_o.transpose(1, 2), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(nloc, O.gather_cf(loc, fidx).transpose(1, 2) + off, rtol=0, atol=0)
    probe = torch.randn(B, S, 3, generator=g).double()
    (off_o.transpose(1, 2) * probe).sum().backward()
    (off * probe).sum().backward()
    torch.testing.assert_close(f2.grad, fea.grad, rtol=1e-10, atol=1e-13)


def test_interp3_cat_ref_equals_the_oracle_in_fp64():
    g = torch.Generator().manual_seed(32)
    B, N, S, C1, C2 = 2, 70, 9, 4, 8
    xyz = (torch.rand(B, 3, N, generator=g) * 2 - 1).double()
    n0 = (torch.rand(B, 3, S, generator=g) * 2 - 1).double()
    n0[:, :, 0] = xyz[:, :, 5]                                         # a node on a point: the clamp is exercised
    p1 = torch.randn(B, C1, N, generator=g).double()
    probe = torch.randn(B, C1 + C2, N, generator=g).double()
    nloc_o, node_o = n0.clone().requires_grad_(True), torch.randn(B, C2, S, generator=g).double().requires_grad_(True)
    out_o = O.upsample_inter(xyz, nloc_o, p1, node_o, 3)               # [B,C1+C2,N]
    (out_o * probe).sum().backward()
    d, idx = O.sqdist_cf(xyz, n0).sort(dim=-1)
    idx3, d3 = idx[:, :, :3], d[:, :, :3]                              # the true fp64 distances
    assert bool((d3 < 1e-10).any())
    nloc = n0.transpose(1, 2).clone().requires_grad_(True)
    node = node_o.detach().transpose(1, 2).clone().requires_grad_(True)
    out = C.interp3_cat_ref(p1.transpose(1, 2), node, xyz.transpose(1, 2), nloc, idx3, d3)
    (out * probe.transpose(1, 2)).sum().backward()
    torch.testing.assert_close(out, out_o.transpose(1, 2), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(node.grad, node_o.grad.transpose(1, 2), rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(nloc.grad, nloc_o.grad.transpose(1, 2), rtol=1e-9, atol=1e-11)
    # the clamped term sends nothing to its node's position: switch every other term's gradient off
    nloc.grad = None
    one = torch.zeros(B, N, C1 + C2, dtype=torch.float64)
    one[:, 5] = 1.0
    (C.interp3_cat_ref(p1.transpose(1, 2), node, xyz.transpose(1, 2), nloc, idx3, d3) * one).sum().backward()
    assert float(nloc.grad[:, 0].abs().max()) == 0.0


@pytest.mark.parametrize('pattern', C.PATTERNS)
def test_node_offset_ref_gradcheck(pattern):
    c = C.node_case(pattern, 2, 11, 4, 5)
    proj = c['proj'].double().requires_grad_(True)
    for k in (0, 1):
        assert torch.autograd.gradcheck(lambda p: C.node_offset_ref(p, c['loc'], c['fidx'], c['gidx'])[k], (proj,))


def test_interp3_cat_ref_gradcheck():
    c = C.interp_case(1, 6, 4, 4, 4)
    d, idx = ((c['xyz'].double()[:, :, None] - c['nloc'].double()[:, None]) ** 2).sum(-1).sort(dim=-1)
    idx3 = idx[:, :, :3]

    def f(fea, node, nloc):       # d3 follows nloc in VALUE here, so that the numeric derivative sees the distance move
        e = ((c['xyz'].double().unsqueeze(2) - C.rows(nloc, idx3)) ** 2).sum(-1)
        return C.interp3_cat_ref(fea, node, c['xyz'], nloc, idx3, e.detach())
    args = tuple(c[k].double().requires_grad_(True) for k in ('fea', 'node', 'nloc'))
    assert torch.autograd.gradcheck(f, args)


def test_fp32_restatement_is_the_same_formula():
    """The fp32 baseline of the bound is the fp64 restatement rounded: close to it, not equal."""
    c = C.node_case('padded', 2, 100, 8, 16)
    r64, r32 = C.node_offset_all(c, torch.float64), C.node_offset_all(c, torch.float32)
    for k in r64:
        assert r32[k].dtype == torch.float32 and 0.0 < C.err(r32[k], r64[k]) < 1e-5, k
    c = C.interp_case(2, 50, 8, 4, 8)
    d, idx = ((c['xyz'][:, :, None] - c['nloc'][:, None]) ** 2).sum(-1).sort(dim=-1)
    r64 = C.interp3_cat_all(c, idx[:, :, :3], d[:, :, :3], torch.float64)
    r32 = C.interp3_cat_all(c, idx[:, :, :3], d[:, :, :3], torch.float32)
    for k in ('out', 'dnode', 'dnloc'):
        assert 0.0 < C.err(r32[k], r64[k]) < 1e-4, k
    assert torch.equal(r64['dfea'], c['g'][:, :, :4].double())


def test_index_patterns():
    B, N, S, ns = 2, 40, 12, 20
    for pattern in C.PATTERNS:
        c = C.node_case(pattern, B, N, S, ns)
        f, g = c['fidx'].long(), c['gidx'].long()
        assert f.shape == (B, S) and g.shape == (B, S, ns) and c['gidx'].dtype == torch.int32
        again = C.node_case(pattern, B, N, S, ns)
        assert all(torch.equal(c[k], again[k]) for k in c)            # a function of the case's name only
        if pattern != 'sentinel':
            assert int(g.min()) >= 0 and int(g.max()) < N and int(f.min()) >= 0 and int(f.max()) < N
        if pattern == 'few':
            assert all(len(set(g[b].flatten().tolist()) | set(f[b].tolist())) <= 5 for b in range(B))
        if pattern == 'padded':
            first = g[:, :, :1]
            tail = (g == first).flip(-1).cumprod(-1).sum(-1)          # length of the trailing run of the first entry
            assert int(tail.max()) == ns and int(tail.min()) >= 1 and len(set(tail.flatten().tolist())) > 3
        if pattern == 'constant':
            assert bool((g == g[:, :, :1]).all()) and bool((f == g[:, :, 0])[:, ::2].all())
        if pattern == 'sentinel':
            assert bool((g[:, ::4] == N).all()) and bool((g[:, 1::4] == N).any()) and bool((g[:, 1::4] == -1).any())
            assert bool((f == N).any()) and bool((f == -1).any())
            assert bool(C.empty_nodes(c)[:, ::4].all()) and not bool(C.empty_nodes(c)[:, 2::4].any())
            named = C.named_points(c)
            assert bool((~named).any()) and bool(named[:, N - 1].all())     # the centre N is clamped to N - 1
            d = C.node_offset_all(c, torch.float64)
            assert float(d['dproj/both'][~named].abs().max()) == 0.0
            assert float(d['off'][C.empty_nodes(c)].abs().max()) == 0.0
