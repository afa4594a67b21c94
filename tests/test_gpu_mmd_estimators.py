"""GPU: mix_rbf_mmd2_and_ratio, linear_mmd2 and poly_mmd2 on HIP (sug_mmd_ratio_* / sug_mmd_adjacent_*, mmd_var.hip) against
the fp64 evaluation of the reference's formulas, with the reference's own fp32 deviation from it (ref_err, recorded in
tests/golden/mmd_estimators.npz) as the second arm of every bound.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import mmd_estimator_cases as C

pytestmark = pytest.mark.gpu
EPS = float(torch.finfo(torch.float32).eps)
CASES = list(range(len(C.ratio_case_ids())))
IDS = C.ratio_case_ids()


def _leaves(ci):
    X, Y = C.ratio_inputs(ci)
    return X.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize('biased', [True, False], ids=['biased', 'unbiased'])
@pytest.mark.parametrize('ci', CASES, ids=IDS)
def test_ratio_values(ci, biased):
    from sug_amd.model import mmd
    G = C.golden()
    X, Y = _leaves(ci)
    with torch.no_grad():
        loss, mmd2, var = (float(v) for v in mmd.mix_rbf_mmd2_and_ratio(X, Y, mmd.sigma_list, biased=biased))
        plain = float(mmd.mix_rbf_mmd2(X, Y, mmd.sigma_list, biased=biased))
    out64, _ = C.ratio_ref64(ci, int(biased))
    l64, m64, v64 = (float(v) for v in out64)
    ref_err = float(G['r%d_b%d_val_err' % (ci, int(biased))][2])
    own = mmd2 / np.sqrt(max(var, 1e-8))                   # fp64, from the kernel's own two fp32 outputs
    ulp = float(np.spacing(np.float32(max(abs(mmd2), abs(plain)))))
    print('%s biased=%d: mmd2 %.8g (fp64 %.8g, mix_rbf_mmd2 %.8g, ulp %.2g)  var_est %.6g (fp64 %.6g, |err| %.2g, ref_err %.2g)  '
          'loss %.8g (own %.8g, fp64 %.8g)' % (IDS[ci], biased, mmd2, m64, plain, ulp, var, v64, abs(var - v64), ref_err, loss, own, l64))
    assert abs(mmd2 - m64) <= 1e-4 * max(1.0, abs(m64))
    assert abs(mmd2 - plain) <= ulp
    assert abs(var - v64) <= max(2.0 * ref_err, 1e-4 * abs(v64))
    assert abs(loss - own) <= 4 * EPS * abs(own)


# ------------------------------------------------------------------------------------------------ 2. gradients
@pytest.mark.parametrize('k', [0, 1, 2], ids=C.UPSTREAMS)
@pytest.mark.parametrize('biased', [True, False], ids=['biased', 'unbiased'])
@pytest.mark.parametrize('ci', CASES, ids=IDS)
def test_ratio_gradients(ci, biased, k):
    """Upstream on loss alone, on mmd2 alone, on var_est alone: wt_m, wt_v and the clamp factor each on their own."""
    from sug_amd.model import mmd
    G = C.golden()
    X, Y = _leaves(ci)
    out = mmd.mix_rbf_mmd2_and_ratio(X, Y, mmd.sigma_list, biased=biased)
    got = torch.cat(torch.autograd.grad(out[k], (X, Y)), 0).cpu().double()
    out64, g64 = C.ratio_ref64(ci, int(biased))
    scale = float(g64[k].abs().max())
    err = float((got - g64[k]).abs().max())
    ref_err = float(G['r%d_b%d_grad_err' % (ci, int(biased))][k])
    print('%s biased=%d d %s: |err| %.3g  scale %.3g  rel %.2g  ref_err %.3g (rel %.2g)' % (
        IDS[ci], biased, C.UPSTREAMS[k], err, scale, err / scale, ref_err, ref_err / scale))
    assert err <= max(2e-4 * scale, 2.0 * ref_err)


@pytest.mark.parametrize('biased', [True, False], ids=['biased', 'unbiased'])
@pytest.mark.parametrize('ci', [ci for ci in CASES if float(C.golden()['r%d_b1_out64' % ci][2]) < 1e-8],
                         ids=[IDS[ci] for ci in CASES if float(C.golden()['r%d_b1_out64' % ci][2]) < 1e-8])
def test_clamped_loss_gradient_is_the_mmd2_gradient_over_sqrt_of_the_floor(ci, biased):
    """var_est < 1e-8: loss = mmd2 / 1e-4 and the clamp passes no gradient to var_est."""
    from sug_amd.model import mmd
    X, Y = _leaves(ci)
    out = mmd.mix_rbf_mmd2_and_ratio(X, Y, mmd.sigma_list, biased=biased)
    assert float(out[2]) < 1e-8
    gl = torch.cat(torch.autograd.grad(out[0], (X, Y), retain_graph=True), 0).double()
    gm = torch.cat(torch.autograd.grad(out[1], (X, Y)), 0).double() * 1e4
    rel = float(((gl - gm).abs() / gm.abs().clamp_min(1e-300)).max())
    print('%s biased=%d: max relative |d loss - 1e4 d mmd2| %.3g (4 eps = %.3g)' % (IDS[ci], biased, rel, 4 * EPS))
    assert bool(((gl - gm).abs() <= 4 * EPS * gm.abs()).all())


# ------------------------------------------------------------------------------------------------ 3. layout and sigmas
@pytest.mark.parametrize('ci', [2, 5, 6], ids=[IDS[2], IDS[5], IDS[6]])       # one tile; partial tiles; the 4 x 4 tiling
def test_row_stride_gives_the_same_bits(ci):
    from sug_amd import ops
    X, Y = C.ratio_inputs(ci)
    m, D = X.shape
    Z = torch.cat((X, Y), 0).cuda()
    wide = torch.full((2 * m, D + 5), 7.0, device='cuda')
    wide[:, :D] = Z
    res = []
    for z in (Z, wide[:, :D]):
        z = z.detach().requires_grad_(True)
        out = ops.mmd_ratio(z, m)
        (g,) = torch.autograd.grad(out[0] + 0.5 * out[1] + 3.0 * out[2], z)
        res.append((torch.stack(out).detach(), g))
    assert not wide[:, :D].is_contiguous()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize('sigmas', [(1.0,), (0.05, 0.1, 0.5, 1, 2, 5, 10, 100)], ids=['nsigma1', 'nsigma8'])
def test_one_and_eight_sigmas(sigmas):
    from sug_amd.model import mmd
    ci = 3
    X, Y = _leaves(ci)
    out = mmd.mix_rbf_mmd2_and_ratio(X, Y, list(sigmas), biased=True)
    got = torch.cat(torch.autograd.grad(out[0], (X, Y)), 0).cpu().double()
    out64, g64 = C.ratio_ref64(ci, 1, tuple(sigmas))
    Xc, Yc = (t.requires_grad_(True) for t in C.ratio_inputs(ci))             # the composed lines in fp32: ref_err
    o32 = mmd.mix_rbf_mmd2_and_ratio(Xc, Yc, list(sigmas), biased=True)
    g32 = torch.cat(torch.autograd.grad(o32[0], (Xc, Yc)), 0).double()
    verr, gerr = abs(float(o32[2]) - float(out64[2])), float((g32 - g64[0]).abs().max())
    scale = float(g64[0].abs().max())
    print('%d sigmas: mmd2 %.8g (fp64 %.8g)  var %.6g (fp64 %.6g, ref_err %.2g)  grad err %.3g scale %.3g ref_err %.3g' % (
        len(sigmas), float(out[1]), float(out64[1]), float(out[2]), float(out64[2]), verr,
        float((got - g64[0]).abs().max()), scale, gerr))
    assert abs(float(out[1]) - float(out64[1])) <= 1e-4 * max(1.0, abs(float(out64[1])))
    assert abs(float(out[2]) - float(out64[2])) <= max(2.0 * verr, 1e-4 * abs(float(out64[2])))
    assert float((got - g64[0]).abs().max()) <= max(2e-4 * scale, 2.0 * gerr)


# ------------------------------------------------------------------------------------------------ 4. capture, reproducibility
@pytest.mark.parametrize('ci', [3, 6], ids=[IDS[3], IDS[6]])
def test_graph_replay_and_repeat_are_bit_identical(ci):
    from sug_amd import ops
    X, Y = C.ratio_inputs(ci)
    m = X.shape[0]
    Znew = torch.cat((X, Y), 0).cuda()

    def run(z):
        out = ops.mmd_ratio(z, m, biased=False)
        (g,) = torch.autograd.grad(out[0] + 0.5 * out[1] + 3.0 * out[2], z)
        return torch.stack(out).detach(), g

    want = run(Znew.clone().requires_grad_(True))
    again = run(Znew.clone().requires_grad_(True))
    assert torch.equal(want[0], again[0]) and torch.equal(want[1], again[1])
    static = (Znew * 0.5 + 0.1).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # (torch's recipe: one warm-up on a side stream before a capture)
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard(), torch.cuda.graph(graph):
        got = run(static)
    with torch.no_grad():
        static.copy_(Znew)
    graph.replay()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 5. linear / poly
@pytest.mark.parametrize('pi', range(len(C.adjacent_params())), ids=['d%g-a%g-c%g' % p for p in C.adjacent_params()])
@pytest.mark.parametrize('si', range(6), ids=['m%d-D%d' % tuple(s) for s in C.golden()['adj_shapes'].tolist()])
def test_linear_and_poly_estimators(si, pi):
    """Integer degrees run on HIP; d = 2.5 takes the composed lines on the device and meets the same bound."""
    from sug_amd import ops
    from sug_amd.model import mmd
    G = C.golden()
    d, alpha, c = C.adjacent_params()[pi]
    X, Y = (t.cuda().requires_grad_(True) for t in C.adjacent_inputs(si))
    assert ops.adjacent_mmd_supported(X, Y, d if d else 1) == float(d).is_integer()
    v = C.adjacent_call(mmd, X, Y, d, alpha, c)
    got = torch.cat(torch.autograd.grad(v, (X, Y)), 0).cpu().double()
    v64, g64 = C.adjacent_ref64(si, pi)
    key = 'a%d_p%d_' % (si, pi)
    verr, gerr = abs(float(G[key + 'v32']) - float(v64)), float(G[key + 'grad_err'])
    scale, err = float(g64.abs().max()), float((got - g64).abs().max())
    print('shape %s d=%g alpha=%g c=%g: value %.8g (fp64 %.8g, ref_err %.2g)  grad err %.3g scale %.3g ref_err %.3g' % (
        tuple(X.shape), d, alpha, c, float(v), float(v64), verr, err, scale, gerr))
    assert abs(float(v) - float(v64)) <= max(1e-4 * max(1.0, abs(float(v64))), 2.0 * verr)
    assert err <= max(2e-4 * scale, 2.0 * gerr)


def test_linear_and_poly_row_stride_and_single_gradient():
    from sug_amd import ops
    X, Y = (t.cuda() for t in C.adjacent_inputs(5))
    wide = torch.zeros(X.shape[0], 2 * X.shape[1], device='cuda')
    wide[:, :X.shape[1]] = Y
    Ys = wide[:, :X.shape[1]]
    for fn in (ops.linear_mmd2, lambda a, b: ops.poly_mmd2(a, b, 3, 0.5, -1.0)):
        Xa, Ya = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        va = fn(Xa, Ya)
        ga = torch.autograd.grad(va, (Xa, Ya))
        Xb = X.clone().requires_grad_(True)
        vb = fn(Xb, Ys)                                   # a strided block that needs no gradient
        (gb,) = torch.autograd.grad(vb, Xb)
        assert torch.equal(va, vb) and torch.equal(ga[0], gb)


# ------------------------------------------------------------------------------------------------ 6. limits
def test_one_row_per_domain_on_the_device():
    from sug_amd import ops
    from sug_amd.model import mmd
    X, Y = torch.randn(1, 4, device='cuda'), torch.randn(1, 4, device='cuda')
    assert torch.isnan(mmd.linear_mmd2(X, Y)) and torch.isnan(mmd.poly_mmd2(X, Y))
    with pytest.raises(ZeroDivisionError):                 # the reference's own end at m = 1 (fixture key ratio_one_row)
        mmd.mix_rbf_mmd2_and_ratio(X, Y, mmd.sigma_list)
    with pytest.raises(RuntimeError, match='m=1'):
        ops.mmd_ratio(torch.cat((X, Y), 0), 1)
    with pytest.raises(RuntimeError):
        ops.poly_mmd2(X.repeat(4, 1), Y.repeat(4, 1), 2.5)
    torch.cuda.synchronize()
