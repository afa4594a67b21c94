"""GPU: the ChamferDistance op (ops.chamfer_nn, sug_amd.chamfer_distance, mmd.cd_distance) -- distances and indices exact
against the fp32 restatement (lowest index on exact ties), gradients against fp64 within the derived bound, independence of
the batch position, hipGraph capture, and the interface.

Worst used share of the gradient bound (K + 6) 2^-24 S seen on the MI355X: 0.26 over the shapes (random and grid clouds),
0.31 in the hub case, 0.22 through cd_distance."""
import pytest
import torch

import chamfer_cases as C

pytestmark = pytest.mark.gpu


def _fwd(a, b):
    from sug_amd import ops
    return ops.chamfer_nn(a.cuda(), b.cuda())


def _assert_forward_exact(a, b, want):
    d1, d2, i1, i2 = _fwd(a, b)
    w1, w2, j1, j2 = want
    assert i1.dtype == torch.int32 and i2.dtype == torch.int32
    assert torch.equal(i1.cpu().long(), j1) and torch.equal(i2.cpu().long(), j2)
    assert torch.equal(d1.cpu(), w1) and torch.equal(d2.cpu(), w2)                 # bit for bit (no NaN in these inputs)


@pytest.mark.parametrize('B,N,M', C.SHAPES)
def test_forward_exact_on_random_clouds(B, N, M):
    a, b, want = C.case('random', B, N, M)
    _assert_forward_exact(a, b, want)


@pytest.mark.parametrize('B,N,M', C.SHAPES)
def test_forward_exact_on_ties(B, N, M):
    """Grid clouds with every point present at least twice: the lowest index of the tied candidates, whatever lanes they fall to."""
    a, b, want = C.case('grid', B, N, M)
    t1, t2 = C.tie_counts(a, b)
    assert (t1 > 0 or M < 2) and (t2 > 0 or N < 2)
    _assert_forward_exact(a, b, want)


@pytest.mark.parametrize('B,N,M', C.SHAPES)
def test_means_agree_with_the_existing_chamfer(B, N, M):
    """dist1.mean(1) + dist2.mean(1) against ops.chamfer: fp32 sums of the same non-negative terms in different orders, each
    within (n - 1) roundings plus the divisions and the final addition: relative (max(N, M) + 8) 2^-24."""
    from sug_amd import ops
    a, b, _ = C.case('random', B, N, M)
    a, b = a.cuda(), b.cuda()
    d1, d2, _, _ = ops.chamfer_nn(a, b)
    got, want = (d1.mean(1) + d2.mean(1)).double(), ops.chamfer(a, b).double()
    rel = ((got - want).abs() / want).max().item()
    print('chamfer_nn means vs ops.chamfer %s: rel %.3g of %.3g' % ((B, N, M), rel, (max(N, M) + 8) * C.U))
    assert rel <= (max(N, M) + 8) * C.U


def _backward(a, b, need_a=True, need_b=True, seed=1):
    from sug_amd import ops
    g = torch.Generator().manual_seed(seed)
    g1, g2 = torch.randn(a.shape[:2], generator=g).cuda(), torch.randn(b.shape[:2], generator=g).cuda()
    A, Bt = a.cuda().requires_grad_(need_a), b.cuda().requires_grad_(need_b)
    d1, d2, i1, i2 = ops.chamfer_nn(A, Bt)
    assert d1.requires_grad and d2.requires_grad and not i1.requires_grad and not i2.requires_grad
    grads = torch.autograd.grad([d1, d2], [t for t in (A, Bt) if t.requires_grad], [g1, g2])
    ga = grads[0] if need_a else None
    gb = grads[-1] if need_b else None
    return (d1.detach(), d2.detach(), i1, i2), (g1, g2), ga, gb


def _share(a, b, fwd, gs, ga, gb):
    r = C.grads_fp64(a, b, fwd[2], fwd[3], gs[0], gs[1])              # the device's own indices
    sa = C.grad_bound_share(ga, r['ga'], r['Ka'], r['Sa']) if ga is not None else 0.0
    sb = C.grad_bound_share(gb, r['gb'], r['Kb'], r['Sb']) if gb is not None else 0.0
    return max(sa, sb), r


@pytest.mark.parametrize('kind', ['random', 'grid'])
@pytest.mark.parametrize('B,N,M', C.SHAPES)
def test_backward_within_the_derived_bound(kind, B, N, M):
    a, b, _ = C.case(kind, B, N, M)
    fwd, gs, ga, gb = _backward(a, b)
    share, _ = _share(a, b, fwd, gs, ga, gb)
    print('chamfer_nn backward %s %s: worst used share of (K + 6) u S = %.3f' % (kind, (B, N, M), share))
    assert share <= 1.0


def test_backward_hub():
    """One point of a is the nearest of all 1021 points of b: K = M on one target, 0 on the others."""
    a, b = C.hub_clouds()
    fwd, gs, ga, gb = _backward(a, b)
    share, r = _share(a, b, fwd, gs, ga, gb)
    Ka = r['Ka'][..., 0]
    assert Ka[0, 0] == 1021 and Ka[1, 37] == 1021 and Ka.sum() == 2 * 1021
    print('chamfer_nn backward hub: worst used share of (K + 6) u S = %.3f' % share)
    assert share <= 1.0


@pytest.mark.parametrize('need_a,need_b', [(True, False), (False, True)])
def test_backward_one_side_only(need_a, need_b):
    a, b, _ = C.case('random', 3, 257, 64)
    fwd, gs, ga, gb = _backward(a, b)
    fwd1, gs1, ga1, gb1 = _backward(a, b, need_a, need_b)
    assert (ga1 is None) == (not need_a) and (gb1 is None) == (not need_b)
    share, _ = _share(a, b, fwd1, gs1, ga1, gb1)
    assert share <= 1.0
    one, both = (ga1, ga) if need_a else (gb1, gb)
    assert torch.equal(one, both)                                      # the same kernel path as with both sides


@pytest.mark.parametrize('N,M', [(257, 64), (1024, 1021)])
def test_independent_of_batch_position_and_run(N, M):
    """A pair alone and the same pair as the second of three: bit-identical distances, indices and gradients; so are two runs."""
    a3, b3 = C.random_clouds(3, N, M, seed=9)
    fwd3, gs3, ga3, gb3 = _backward(a3, b3)
    again = _backward(a3, b3)
    for x, y in zip(fwd3 + (ga3, gb3), again[0] + (again[2], again[3])):
        assert torch.equal(x, y)
    from sug_amd import ops
    A, Bt = a3[1:2].cuda().requires_grad_(True), b3[1:2].cuda().requires_grad_(True)
    d1, d2, i1, i2 = ops.chamfer_nn(A, Bt)
    ga, gb = torch.autograd.grad([d1, d2], [A, Bt], [gs3[0][1:2].contiguous(), gs3[1][1:2].contiguous()])
    for alone, batched in zip((d1, d2, i1, i2, ga, gb), fwd3 + (ga3, gb3)):
        assert torch.equal(alone.detach(), batched[1:2])


def test_captured_forward_and_backward_replay_bit_for_bit():
    """cd_distance(batch_loss=False) forward + backward in one torch.cuda.graph on one stream, replayed on two further inputs."""
    from sug_amd import ops
    from sug_amd.chamfer_distance import ChamferDistance
    from sug_amd.model import mmd
    cd = ChamferDistance()
    inputs = [C.random_clouds(3, 257, 64, seed=s) for s in (5, 6, 7)]

    def run(x1, x2):
        loss = mmd.cd_distance(x1, x2, cd, batch_loss=False)
        return (loss,) + torch.autograd.grad(loss, [x1, x2])

    s1, s2 = (t.cuda().requires_grad_(True) for t in inputs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # torch's recipe: one warm-up on a side stream
        run(s1, s2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard(), torch.cuda.graph(graph):
        got = run(s1, s2)
    for x1, x2 in inputs[1:]:
        with torch.no_grad():
            s1.copy_(x1)
            s2.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        want = run(x1.cuda().requires_grad_(True), x2.cuda().requires_grad_(True))
        for g, w in zip(got, want):
            assert torch.equal(g.detach(), w.detach())


def test_module_returns_int64_indices_without_grad():
    from sug_amd.chamfer_distance import ChamferDistance, chamfer_distance
    a, b, want = C.case('grid', 3, 65, 9)
    x1, x2 = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    for f in (ChamferDistance(), chamfer_distance):
        d1, d2, i1, i2 = f(x1, x2)
        assert i1.dtype == torch.int64 and i2.dtype == torch.int64 and not i1.requires_grad and not i2.requires_grad
        assert d1.requires_grad and d2.requires_grad
        assert torch.equal(i1.cpu(), want[2]) and torch.equal(i2.cpu(), want[3])
        assert torch.equal(d1.detach().cpu(), want[0]) and torch.equal(d2.detach().cpu(), want[1])


@pytest.mark.parametrize('batch_loss', [True, False])
def test_cd_distance_both_branches(batch_loss):
    """Loss and gradients of mmd.cd_distance against the fp64 restatement by the device's indices.  The upstream gradients
    that autograd hands to the op are read off the graph (fp32, as the kernel gets them), so the gradient bound is the op's
    own (K + 6) 2^-24 S; the loss is a mean of non-negative fp32 terms: relative (max(N, M) + 8) 2^-24."""
    from sug_amd.chamfer_distance import ChamferDistance
    from sug_amd.model import mmd
    B, N, M = 3, 257, 64
    a, b, _ = C.case('random', B, N, M)
    x1, x2 = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    seen = []
    cd = ChamferDistance()

    def recording(p1, p2):
        seen.append(cd(p1, p2))
        return seen[-1]

    loss = mmd.cd_distance(x1, x2, recording, batch_loss=batch_loss)
    assert loss.shape == ((B,) if batch_loss else ())
    w = torch.rand(B, generator=torch.Generator().manual_seed(4)).cuda() + 0.5 if batch_loss else torch.ones((), device='cuda')
    d1, d2, i1, i2 = seen[0]
    g1, g2, ga, gb = torch.autograd.grad((loss * w).sum(), [d1, d2, x1, x2])
    r = C.grads_fp64(a, b, i1, i2, g1, g2)
    ref = r['dist1'].mean(1) + r['dist2'].mean(1) if batch_loss else r['dist1'].mean() + r['dist2'].mean()
    assert bool(((loss.detach().cpu().double() - ref).abs() <= (max(N, M) + 8) * C.U * ref).all())
    share = max(C.grad_bound_share(ga, r['ga'], r['Ka'], r['Sa']), C.grad_bound_share(gb, r['gb'], r['Kb'], r['Sb']))
    print('cd_distance(batch_loss=%s): worst used share %.3f' % (batch_loss, share))
    assert share <= 1.0


def test_geometric_weights_keep_their_path():
    from sug_amd import ops
    from sug_amd.model import mmd
    a, b, _ = C.case('random', 3, 257, 64)
    a, b = a.cuda(), b.cuda()
    for weighting in ('naive_inverse', 'exp_inverse', 'mean2one'):
        assert torch.equal(mmd.geometric_weights(a, b, weighting=weighting), ops.chamfer_weights(a, b, weighting).reshape(1, -1))
    assert torch.equal(mmd.chamfer_distances(a, b), ops.chamfer(a, b))
    cf = a.transpose(1, 2).unsqueeze(-1).contiguous(), b.transpose(1, 2).unsqueeze(-1).contiguous()   # [m,3,N,1] as the trainer passes
    assert torch.equal(mmd.geometric_weights(*cf, weighting='mean2one'), ops.chamfer_weights(a, b, 'mean2one').reshape(1, -1))


def test_refusals():
    from sug_amd import ops
    from sug_amd.chamfer_distance import ChamferDistance
    cd = ChamferDistance()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device='cuda')
    for f in (ops.chamfer_nn, cd):
        with pytest.raises(RuntimeError, match='fp32'):
            f(z(2, 8, 3, dtype=torch.float16), z(2, 8, 3, dtype=torch.float16))
        with pytest.raises(RuntimeError, match=r'\[B,N,3\]'):
            f(z(2, 8, 2), z(2, 8, 2))
        with pytest.raises(RuntimeError, match='paired'):
            f(z(2, 8, 3), z(3, 8, 3))
        with pytest.raises(RuntimeError, match='5000'):
            f(z(1, 5001, 3), z(1, 8, 3))
        with pytest.raises(RuntimeError, match='5000'):
            f(z(1, 8, 3), z(1, 5001, 3))
