"""GPU: the forward of the SA-node module's pass-invariant half (offset projection, residual layer) run once per step
(every pass keeps its own backward through it), and both passes' glue (node_offset -> knn_query -> group_max -> three_nn ->
interp3_cat) in one launch per stage.

1. the entry points over 2B pass-major virtual clouds equal two per-pass calls bit for bit;
2. a step with the half shared equals the recomputing form (losses and BatchNorm buffers bit for bit, gradients at the
   bound tests/test_gpu_step.py::test_prefix_sharing_is_exact fixes for a change of summation order: rtol 1e-4,
   atol 3e-6 * max|grad|);
3. the fallbacks (no geometry plan; the four-call form of a plain Net_MDA; a weight changed between the passes);
4. a captured SUGStep follows the eager one."""
import hashlib

import pytest
import torch

from conftest import load_golden
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the entry points
@pytest.mark.parametrize('B', [3, 8])          # 3: odd, not a multiple of 8 (plain block mapping); 8: the XCD mapping
def test_batched_glue_equals_per_pass_glue(B):
    from sug_amd import ops
    N, S, ns, C = 160, 64, 64, 64               # N no multiple of 64
    g = torch.Generator().manual_seed(5)
    loc = O.synth_clouds(B, N, g).squeeze(-1).transpose(1, 2).contiguous()
    loc[1] *= 3.0                               # a sparse cloud: its balls of radius 0.3 hold few points
    loc = loc.cuda()
    proj = torch.randn(B, N, 3, generator=g).cuda()
    res = torch.randn(B, N, C, generator=g).cuda()
    fea = torch.randn(B, N, C, generator=g).cuda()
    starts = torch.cat([torch.randint(0, N, (B,), generator=g), torch.randint(0, N, (B,), generator=g)])
    assert not torch.equal(starts[:B], starts[B:])
    locp = loc.repeat(2, 1, 1)
    fidx = ops.fps(locp, S, starts)
    f_loc = ops.gather_rows(locp, fidx)
    gidx = ops.ball_query(locp, f_loc, 0.3, ns)
    assert not torch.equal(fidx[:B], fidx[B:])
    hits = ((f_loc[1][:, None, :] - loc[1][None, :, :]) ** 2).sum(-1).le(0.3 ** 2).sum(1)
    assert int(hits.min()) < ns, 'the case needs a ball with fewer than ns hits'
    got = ops.sa_glue_passes(proj, res, fea, locp, fidx, gidx, 64)
    assert got['out'].shape == (2 * B, N, 2 * C) and got['node'].shape == (2 * B, S, C)
    for p in range(2):
        sl = slice(p * B, (p + 1) * B)
        off, nloc = ops.node_offset(proj, loc, fidx[sl], gidx[sl])
        gidx2 = ops.knn_query(loc, nloc, 64)
        node, arg = ops._group_max_raw(res, C, B, gidx2, N, C)
        idx3, d3 = ops.three_nn_raw(loc, nloc)
        out = ops.interp3_cat(fea, node, loc, nloc)
        want = {'off': off, 'nloc': nloc, 'gidx2': gidx2, 'node': node, 'arg': arg, 'idx3': idx3, 'd3': d3, 'out': out}
        assert want.keys() == got.keys()
        for k, v in want.items():
            assert torch.equal(got[k][sl], v), (p, k)
    assert not torch.equal(got['out'][:B], got['out'][B:])          # the passes do differ


def test_shared_entry_points_refuse_partial_passes():
    from sug_amd import ops
    proj = torch.zeros(2, 8, 3).cuda()
    loc = torch.zeros(3, 8, 3).cuda()
    fidx = torch.zeros(3, 4, dtype=torch.int32).cuda()
    gidx = torch.zeros(3, 4, 4, dtype=torch.int32).cuda()
    with pytest.raises(RuntimeError, match='whole passes'):
        ops._node_offset_raw(proj, loc, fidx, gidx)
    with pytest.raises(RuntimeError, match='whole passes'):
        ops._group_max_raw(torch.zeros(2, 8, 4).cuda(), 4, 2, gidx, 8, 4)


# ------------------------------------------------------------------------------------------------ 2./3. a step
def _net(seed):
    from sug_amd.model.Model import Net_MDA
    net = Net_MDA('DGCNN')
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    return net.cuda().train()


_STEPS = {}


def _step(pair, share, plan='1', batched='1'):
    """One SUGStep.losses + backward on the golden batch -> (losses, grads, BatchNorm buffers, batched-glue calls); computed
    once per form and shared by the tests below (nobody changes it)."""
    key = (pair, share, plan, batched)
    if key in _STEPS:
        return _STEPS[key]
    from sug_amd import ops
    from sug_amd.model import model_utils
    from sug_amd.train_step import SUGStep
    G = load_golden('step_dgcnn.npz')
    seed = G['seed']
    mp = pytest.MonkeyPatch()
    calls = [0]
    real = ops.sa_glue_passes

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    try:
        mp.setenv('SUG_PLAN_GEOMETRY', plan)
        mp.setattr(model_utils, 'SA_GLUE_BATCHED', batched == '1')
        mp.setattr(ops, 'sa_glue_passes', spy)
        net = _net(seed)
        tr = SUGStep(net, share_prefix=share, fused_adam=False, pair_domains=pair)
        torch.manual_seed(seed)
        lc, lg, ls = tr.losses(G['data'].cuda(), G['label'].cuda(), G['data_t'].cuda(), G['label_t'].cuda())
        (lc + lg + ls).backward()
    finally:
        mp.undo()
    _STEPS[key] = ([lc.item(), lg.item(), ls.item()],
                   {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None},
                   {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k}, calls[0])
    return _STEPS[key]


def _same_step(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert a[1].keys() == b[1].keys()
    gmax = max(float(g.abs().max()) for g in a[1].values())
    for k in a[1]:
        print(k, 'max |d grad| %.3e of gmax %.3e' % (float((a[1][k] - b[1][k]).abs().max()), gmax))
    for k in a[1]:
        torch.testing.assert_close(b[1][k], a[1][k], rtol=1e-4, atol=3e-6 * gmax)
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize('pair', [True, False])
def test_shared_step_equals_unshared_step(pair):
    plain, shared = _step(pair, False), _step(pair, True)
    _same_step(plain, shared)
    for r in (plain, shared):       # one train-mode forward per domain and pass, replayed or run
        assert int(r[2]['g.node_fea_adapt.residual.conv.1.num_batches_tracked']) == 4
        assert int(r[2]['g.conv1.conv.1.num_batches_tracked']) == 4
    # both passes' glue in one set of launches exactly where a two-pass plan exists and the half is shared
    assert plain[3] == 0 and shared[3] == (1 if pair else 0)


def test_residual_counter_advances_by_two_per_step_and_domain():
    """Per domain group the residual BatchNorm sees the semantic and the node pass: 2 per step (4 over both domains)."""
    from sug_amd import ops
    net = _net(3)
    G = load_golden('step_dgcnn.npz')
    net.g.share_prefix = True
    bn = net.g.node_fea_adapt.residual.conv[1]
    x = G['data'].cuda()
    with torch.no_grad():
        net(x, semantic_adaption=True)
        assert int(bn.num_batches_tracked) == 1
        net(x, node_adaptation_s=True)
    assert int(bn.num_batches_tracked) == 2
    assert ops.CTX.bn_groups == 1


def test_without_a_plan_the_half_is_still_shared():
    planned, unplanned = _step(True, True), _step(True, True, plan='0')
    assert unplanned[3] == 0
    # the geometric MMD term carries the Chamfer weights, whose float atomics are not ordered (the bound
    # test_planned_geometry_of_both_passes_is_the_same_step holds the two forms to)
    assert planned[0][0] == unplanned[0][0] and planned[0][2] == unplanned[0][2], (planned[0], unplanned[0])
    assert abs(planned[0][1] - unplanned[0][1]) <= 1e-6 * abs(unplanned[0][1])
    for k in planned[2]:
        assert torch.equal(planned[2][k], unplanned[2][k]), k
    gmax = max(float(g.abs().max()) for g in planned[1].values())
    for k in planned[1]:
        torch.testing.assert_close(planned[1][k], unplanned[1][k], rtol=1e-4, atol=3e-6 * gmax)
    _same_step(_step(True, False, plan='0'), unplanned)


def test_per_pass_glue_switch_is_the_same_step():
    a, b = _step(True, True), _step(True, True, batched='0')
    assert b[3] == 0
    assert a[0] == b[0]
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[1]:                  # the same kernels on the same values in the same order, forward and backward
        assert torch.equal(a[1][k], b[1][k]), k


def _four_calls(net, G):
    from sug_amd.model import mmd
    data, data_t, lab, lab_t = G['data'].cuda(), G['data_t'].cuda(), G['label'].cuda(), G['label_t'].cuda()
    cfg = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 50, 'GEO_SCALE': 1}
    ys = net(data, semantic_adaption=True)
    yt = net(data_t, semantic_adaption=True)
    fs = net(data, node_adaptation_s=True)
    ft = net(data_t, node_adaptation_t=True)
    lc = torch.nn.functional.cross_entropy(ys[0], lab)
    lg = mmd.mmd_cal(lab, fs, lab_t, ft, cfg)
    ls = mmd.mmd_cal(lab, ys[2], lab_t, yt[2], cfg)
    (lc + lg + ls).backward()
    return ([lc.item(), lg.item(), ls.item()], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None},
            {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k}, 0)


def test_four_call_form_shares_the_half(monkeypatch):
    """A plain Net_MDA (share_prefix 'auto'), four forwards and one backward: the residual layer's forward runs once per
    batch."""
    G = load_golden('step_dgcnn.npz')
    res, runs = [], []
    for mode in (False, 'auto'):
        net = _net(G['seed'])
        net.g.share_prefix = mode
        n = [0]
        real = net.g.node_fea_adapt.residual.rows

        def spy(x, pre=None, keep=None, real=real, n=n):
            n[0] += pre is None                 # a forward that is computed, not taken over
            return real(x, pre=pre, keep=keep)
        monkeypatch.setattr(net.g.node_fea_adapt.residual, 'rows', spy)
        torch.manual_seed(G['seed'])
        res.append(_four_calls(net, G))
        runs.append(n[0])
    assert runs == [4, 2], runs
    _same_step(res[0], res[1])
    assert int(res[1][2]['g.node_fea_adapt.residual.conv.1.num_batches_tracked']) == 4


def test_a_weight_changed_between_the_passes_is_seen(monkeypatch):
    """The cache key counts the versions of the residual layer's and the offset projection's parameters: an in-place
    change between the semantic and the node pass makes the node pass recompute, and it computes what the unshared
    form computes."""
    G = load_golden('step_dgcnn.npz')
    x = G['data'].cuda()
    outs, runs = [], []
    for mode, touch in ((False, True), ('auto', True), ('auto', False)):
        net = _net(G['seed'])
        net.g.share_prefix = mode
        n = [0]
        real = net.g.node_fea_adapt.residual.rows

        def spy(t, pre=None, keep=None, real=real, n=n):
            n[0] += pre is None                 # a forward that is computed, not taken over
            return real(t, pre=pre, keep=keep)
        monkeypatch.setattr(net.g.node_fea_adapt.residual, 'rows', spy)
        torch.manual_seed(G['seed'])
        net(x, semantic_adaption=True)
        if touch:
            with torch.no_grad():
                net.g.node_fea_adapt.residual.conv[0].weight.mul_(0.5)
        outs.append(net(x, node_adaptation_s=True).detach())
        runs.append(n[0])
    assert runs == [2, 2, 1], runs
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[1], outs[2])


# ------------------------------------------------------------------------------------------------ 4. captured = eager
def _sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_captured_step_equals_eager_step():
    from sug_amd.train_step import SUGStep
    B, N = 2, 128
    g = torch.Generator().manual_seed(17)
    data, data_t = O.synth_clouds(B, N, g).cuda(), O.synth_clouds(B, N, g).cuda()
    lab, lab_t = torch.randint(0, 10, (B,), generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()
    res = []
    for use_graph in (False, True):
        net = _net(17)
        tr = SUGStep(net, use_graph=use_graph)
        assert tr.share_prefix and tr.pair_domains
        torch.manual_seed(17)
        out = [[float(v) for v in tr.step(data, lab, data_t, lab_t)] for _ in range(3)]
        torch.cuda.synchronize()
        res.append((out, _sha(net.state_dict())))
        if use_graph:
            (st,) = tr._graphs.values()
            assert st['graph'] is not None, 'the step was not captured'
            # one FPS start draw per pass over the paired batch, as before the glue of both passes shared its launches
            assert st['feeder'].plan == [(2 * B, N), (2 * B, N)], st['feeder'].plan
    assert res[0][0] == res[1][0], res
    assert res[0][1] == res[1][1]
