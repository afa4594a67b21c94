"""One launch per stage instead of one per domain group / attention layer / direction: the bn5 stage under bn_groups(G)
(sug_bn_act_pool_groups_fwd / _bwd, sug_col_stats_bn_groups_exact), the two CALayers' gate + BatchNorm
(sug_gate_bn_fwd_multi / _bwd_multi) and the two Chamfer directions (sug_chamfer_merged, sug_chamfer_weights_merged).
Each merged form must give the BITS of the launch-per-group form, which the module switches of ops.py (BN_POOL_GROUPED,
GATE_BN_MULTI, CHAMFER_MERGED) still select; the bn5 stage is also anchored to a plain torch fp64 composition."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _switch(name, value):
    from sug_amd import ops
    old = getattr(ops, name)
    setattr(ops, name, value)
    try:
        yield
    finally:
        setattr(ops, name, old)


def _bn(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        w = 1 + 0.3 * torch.randn(C, generator=g)
        w[::4] = -w[::4]                               # negative scales: the max picks the smallest input
        bn.weight.copy_(w)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn.cuda().train()


def _bn5_input(shape, G, seed):
    B, N, C = shape
    y = torch.randn(B, N, C, generator=torch.Generator().manual_seed(seed)) + 0.3
    if G > 1:
        y[B // G:2 * (B // G)] += 3.0                  # unequal group means: a group's coefficients used on another shows
    return y.cuda()


def _bn5_stage(y, G, merged, seed):
    """The bn5 stage twice (pooling forward, then the buffers-only update of the node pass), then the pooling backward.
    -> dict of everything the stage produces."""
    from sug_amd import ops
    B, N, C = y.shape
    bn = _bn(C, seed)
    probe = torch.randn(B, 2 * C, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    yi = y.clone().requires_grad_(True)
    with _switch('BN_POOL_GROUPED', merged), ops.bn_groups(G):
        pooled = ops.bn_act_pool_cat(yi, bn, 0.2)
        _, coef, arg = pooled.grad_fn.saved_tensors    # what the forward keeps for the backward
        ops.bn_update_stats(y, bn)
        (pooled * probe).sum().backward()
    return {'pooled': pooled.detach(), 'arg': arg, 'coef': coef, 'running_mean': bn.running_mean,
            'running_var': bn.running_var, 'num_batches_tracked': bn.num_batches_tracked, 'dy': yi.grad,
            'dgamma': bn.weight.grad, 'dbeta': bn.bias.grad, 'probe': probe}


_FULL = {}


def _full_size(merged):
    """[16, 1024, 512] in 2 groups: 8192 rows per group, the smallest size at which cutting the rows of BOTH groups into one
    workspace (18 rows per workgroup) differs from cutting each group on its own (10).  Computed once per form."""
    if merged not in _FULL:
        _FULL[merged] = _bn5_stage(_bn5_input((16, 1024, 512), 2, 11), 2, merged, 21)
    return _FULL[merged]


def _assert_same_bits(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k], b[k]), '%s differs: max |d| = %g' % (k, float((a[k].double() - b[k].double()).abs().max()))


def test_bn5_stage_full_size_has_the_bits_of_the_per_group_launches():
    a, b = _full_size(True), _full_size(False)
    assert int(a['num_batches_tracked']) == 4          # two calls of two groups
    _assert_same_bits(a, b)


@pytest.mark.parametrize('shape,G', [((6, 100, 64), 2), ((6, 100, 64), 3), ((4, 64, 512), 1)])
def test_bn5_stage_small_has_the_bits_of_the_per_group_launches(shape, G):
    """N = 100 is no multiple of the row lanes of any kernel of the stage; three groups; one group (path unchanged)."""
    y = _bn5_input(shape, G, 5)
    _assert_same_bits(_bn5_stage(y, G, True, 7), _bn5_stage(y, G, False, 7))


def test_bn5_stage_full_size_against_fp64():
    """The merged form against BatchNorm (batch statistics per group) -> LeakyReLU(0.2) -> max | mean in plain torch fp64,
    at the tolerances test_gpu_edgeconv.py::test_bn_act_pool_vs_torch uses for this op against the fp32 composition."""
    res = _full_size(True)
    y = _bn5_input((16, 1024, 512), 2, 11).double()
    B, N, C = y.shape
    bn = _bn(C, 21).double()
    yr = y.clone().requires_grad_(True)
    for rep in range(2):                               # the pooling pass, then the buffers-only pass: four updates
        parts = []
        for part in yr.chunk(2, dim=0):
            parts.append(F.leaky_relu(F.batch_norm(part.reshape(-1, C), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                                                   True, 0.1, 1e-5), 0.2).view(B // 2, N, C))
    r = torch.cat(parts)
    ref = torch.cat((r.max(dim=1)[0], r.mean(dim=1)), 1)
    (ref * res['probe'].double()).sum().backward()
    torch.testing.assert_close(res['pooled'][:, :C].double(), ref[:, :C], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(res['pooled'][:, C:].double(), ref[:, C:], rtol=1e-4, atol=1e-5)
    at_arg = r.detach().gather(1, res['arg'].long()[:, None, :]).squeeze(1)      # (two points within fp32 rounding of each other may swap)
    torch.testing.assert_close(at_arg, ref[:, :C].detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(res['dy'].double(), yr.grad, rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(res['dgamma'].double(), bn.weight.grad, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(res['dbeta'].double(), bn.bias.grad, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(res['running_mean'].double(), bn.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(res['running_var'].double(), bn.running_var, rtol=1e-5, atol=1e-6)


def _calayers(M, nl, multi):
    from sug_amd import ops
    from sug_amd.model.Model import CALayer
    g = torch.Generator().manual_seed(100 * M + nl)
    C = 4096
    mods = []
    for a in range(nl):                                # different weights, scales and running buffers per layer
        m = CALayer(C)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.02 if p.dim() > 1 else 0.3))
            m.bn.weight.add_(1.0 + a)
            m.bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
            m.bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        mods.append(m.cuda().train())
    x = (torch.randn(nl * M, C, generator=g)).cuda().requires_grad_(True)
    probe = torch.randn(nl * M, C, generator=g).cuda()
    with _switch('GATE_BN_MULTI', multi):
        assert ops.calayer_supported(tuple(mods), x)
        out = ops.calayers(tuple(mods), x)
        (out * probe).sum().backward()
    res = {'out': out.detach(), 'dx': x.grad}
    for a, m in enumerate(mods):
        res['rm%d' % a], res['rv%d' % a], res['nbt%d' % a] = m.bn.running_mean, m.bn.running_var, m.bn.num_batches_tracked
        for k, p in m.named_parameters():
            res['%d.%s' % (a, k)] = p.grad
    return res


@pytest.mark.parametrize('M,nl', [(4, 2), (32, 2), (32, 1)])
def test_calayers_one_launch_for_both_layers_has_the_bits_of_the_loop(M, nl):
    """M = 4: rows short of the 32 kept in registers; M = 32: the step's size; one layer: the call is unchanged."""
    a, b = _calayers(M, nl, True), _calayers(M, nl, False)
    assert all(v is not None for v in a.values())
    _assert_same_bits(a, b)


@pytest.mark.parametrize('B,N,M', [(3, 64, 48), (32, 64, 64)])
def test_chamfer_both_directions_in_one_launch_has_the_bits_of_two(B, N, M):
    """N != M: swapped operands, an LDS size or a partial-row length taken from the wrong direction would show."""
    from sug_amd import ops
    g = torch.Generator().manual_seed(B + N)
    a, b = torch.rand(B, N, 3, generator=g).cuda(), (torch.rand(B, M, 3, generator=g) * 1.5).cuda()
    res = []
    for merged in (True, False):
        with _switch('CHAMFER_MERGED', merged):
            res.append([ops.chamfer(a, b)] + [ops.chamfer_weights(a, b, m) for m in ('naive_inverse', 'exp_inverse', 'mean2one')])
    for x, y in zip(*res):
        assert x.shape == (B,) and torch.equal(x, y)
    # and against the definition, so that equality with the two-launch form is not the only anchor
    d = ((a.double()[:, :, None] - b.double()[:, None]) ** 2).sum(-1)
    ref = d.min(2)[0].mean(1) + d.min(1)[0].mean(1)
    torch.testing.assert_close(res[0][0].double(), ref, rtol=1e-5, atol=1e-7)
