"""GPU parity of the fused Point Transformer attention (sug_ptran_* kernels + hand-written backward) against
the same block composed of separate torch / gather ops in the reference's order
(model/Ptran_transformer.py:32-45): fp32 mode 1e-4 (north star), fp16 mode reported and bounded."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _block(d_points, seed):
    from sug_amd.model.Ptran_transformer import TransformerBlock
    torch.manual_seed(seed)
    blk = TransformerBlock(d_points, 512, 16).cuda()
    return blk


def _run(blk, xyz, feat, probe, fused):
    for p in blk.parameters():
        p.grad = None
    f = feat.clone().requires_grad_(True)
    out, attn = blk(xyz, f, need_attn=not fused)
    assert (attn is None) == fused
    (out * probe).sum().backward()
    grads = {k: v.grad.clone() for k, v in blk.named_parameters()}
    return out.detach(), f.grad.clone(), grads


@pytest.mark.parametrize('B,n,dp', [(2, 300, 64), (3, 16, 128), (2, 4, 512), (1, 1024, 32)])
def test_fused_attention_fp32_matches_composition(B, n, dp):
    blk = _block(dp, 1)
    g = torch.Generator().manual_seed(n)
    xyz = torch.rand(B, n, 3, generator=g).cuda()
    feat = torch.randn(B, n, dp, generator=g).cuda()
    probe = torch.randn(B, n, dp, generator=g).cuda()
    o1, gf1, gr1 = _run(blk, xyz, feat, probe, True)
    o0, gf0, gr0 = _run(blk, xyz, feat, probe, False)
    torch.testing.assert_close(o1, o0, rtol=1e-4, atol=1e-4)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-12))
    assert rel(gf1, gf0) < 1e-4, rel(gf1, gf0)
    gmax = max(float(v.norm()) for v in gr0.values())
    for k in gr0:       # (fc_gamma.2.bias has zero gradient identically: a per-channel shift cancels in the softmax)
        assert float((gr1[k] - gr0[k]).norm()) <= 2e-4 * float(gr0[k].norm()) + 1e-6 * gmax, (k, rel(gr1[k], gr0[k]))


def test_fused_attention_fp16_mode_deviation():
    """BASELINE config 5's 16-bit mode: the k-expanded tensors and the three 512 x 512 linears in fp16
    (MFMA, fp32 accumulation); softmax statistics, q / K / V, reductions in fp32."""
    from sug_amd.model import Ptran_transformer as PT
    blk = _block(64, 2)
    g = torch.Generator().manual_seed(5)
    B, n = 2, 512
    xyz = torch.rand(B, n, 3, generator=g).cuda()
    feat = torch.randn(B, n, 64, generator=g).cuda()
    probe = torch.randn(B, n, 64, generator=g).cuda()
    o0, gf0, gr0 = _run(blk, xyz, feat, probe, True)
    try:
        PT.GEMM_DTYPE = torch.float16
        o1, gf1, gr1 = _run(blk, xyz, feat, probe, True)
    finally:
        PT.GEMM_DTYPE = None
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-12))
    dev = {'out': rel(o1, o0), 'dfeat': rel(gf1, gf0), **{k: rel(gr1[k], gr0[k]) for k in gr0 if k != 'fc_gamma.2.bias'}}
    print('fp16 mode, relative L2 deviation from fp32:', {k: '%.2e' % v for k, v in dev.items()})
    assert dev['out'] < 2e-3 and dev['dfeat'] < 2e-2
    assert all(v < 5e-2 for v in dev.values()), dev


def test_linear16_matches_fp32_linear_to_fp16_rounding():
    """ops.linear16 (16-bit operands, fp32 accumulation, fp32 results and parameter gradients without cast kernels):
    values and gradients within fp16 operand rounding of nn.Linear in fp32."""
    from sug_amd import ops
    g = torch.Generator().manual_seed(2)
    lin = torch.nn.Linear(96, 160).cuda()
    x = torch.randn(3, 700, 96, generator=g).cuda().requires_grad_(True)
    probe = torch.randn(3, 700, 160, generator=g).cuda()
    y0 = lin(x)
    g0 = torch.autograd.grad((y0 * probe).sum(), (x, lin.weight, lin.bias))
    y1 = ops.linear16(x, lin, torch.float16)
    assert y1.dtype == torch.float32
    g1 = torch.autograd.grad((y1 * probe).sum(), (x, lin.weight, lin.bias))
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(y1, y0) < 2e-3
    assert all(a.dtype == torch.float32 for a in g1)
    assert rel(g1[0], g0[0]) < 2e-3 and rel(g1[1], g0[1]) < 2e-3 and rel(g1[2], g0[2]) < 1e-5
    # 16-bit output for a following 16-bit GEMM
    y2 = ops.linear16(x, lin, torch.float16, out32=False)
    assert y2.dtype == torch.float16 and rel(y2.float(), y0) < 3e-3


@pytest.mark.parametrize('B,n', [(2, 512), (1, 2048), (3, 16), (2, 64)])
def test_one_kernel_fp16_forward_matches_the_composed_fp16_chain(B, n):
    """Round 6 (BASELINE config 5: "fp16 with MFMA attention path"): sug_ptran_fused_fwd -- pos1, the three 512 x 512 linears
    on v_mfma_f32_32x32x16_f16 with the activations resident in LDS, q - k + delta, softmax over the 16 neighbours, weighted
    sum -- against the same fp16 chain composed of sug_ptran_pos1 / qk / attn and three library GEMMs (ops.PTRAN_FUSED = False).
    Both round the k-expanded tensors to fp16 at the same points and accumulate in fp32; they differ by the order of the
    GEMMs' partial sums only: outputs within 2e-3 (relative L2 3e-4), every saved tensor within fp16 rounding of the
    other's, and -- the backward being the same code fed with those tensors -- gradients within 2e-3 relative L2."""
    from sug_amd import ops
    from sug_amd.model import Ptran_transformer as PT
    blk = _block(64, 3)
    g = torch.Generator().manual_seed(B * 1000 + n)
    xyz = torch.rand(B, n, 3, generator=g).cuda()
    feat = torch.randn(B, n, 64, generator=g).cuda()
    probe = torch.randn(B, n, 64, generator=g).cuda()
    assert ops.lib().sug_ptran_fused_supported(B, n, min(16, n), 512) == 1
    res = {}
    keep = ops.PTRAN_FUSED
    try:
        PT.GEMM_DTYPE = torch.float16
        for fused in (True, False):
            ops.PTRAN_FUSED = fused
            res[fused] = _run(blk, xyz, feat, probe, True)
        # without a backward (torch.no_grad): the kernel's save = 0 form, same values
        ops.PTRAN_FUSED = True
        with torch.no_grad():
            o_ng = blk(xyz, feat)[0]
    finally:
        PT.GEMM_DTYPE, ops.PTRAN_FUSED = None, keep
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-12))
    (o1, gf1, gr1), (o0, gf0, gr0) = res[True], res[False]
    assert torch.equal(o_ng, o1), 'save = 0 and save = 1 must give the same output'
    assert rel(o1, o0) < 3e-4, rel(o1, o0)
    torch.testing.assert_close(o1, o0, rtol=2e-3, atol=2e-3)
    assert rel(gf1, gf0) < 2e-3, rel(gf1, gf0)
    gmax = max(float(v.norm()) for v in gr0.values())
    for k in gr0:
        assert float((gr1[k] - gr0[k]).norm()) <= 2e-3 * float(gr0[k].norm()) + 1e-5 * gmax, (k, rel(gr1[k], gr0[k]))


def test_one_kernel_forward_is_declined_where_it_does_not_apply():
    """k < 16 (a level with fewer than 16 points) and point counts that are not whole octets take the composed chain."""
    from sug_amd import ops
    L = ops.lib()
    assert L.sug_ptran_fused_supported(2, 4, 4, 512) == 0
    assert L.sug_ptran_fused_supported(1, 20, 16, 512) == 0
    assert L.sug_ptran_fused_supported(2, 2048, 16, 512) == 1


# ----------------------------------------------------------------------------- against fp64, in the peaked regime
# The comparisons above hold the fused path against a composition of the project's own ops under the default
# initialisation, where every softmax weight is within 2 % of 1/16.  Below, fc_gamma[2] is multiplied by a gain (256:
# weights 6e-4 .. 0.78, 1024: 1e-11 .. 1.0, the regime of a trained network) and the reference is the plain fp64
# restatement of tests/ptran_kernel_cases.py on the CPU, on the neighbour lists the block itself found.
import functools  # noqa: E402

import ptran_kernel_cases as C  # noqa: E402


def _gained_block(dp, seed, gain):
    blk = _block(dp, seed)
    with torch.no_grad():
        blk.fc_gamma[2].weight *= gain
        blk.fc_gamma[2].bias *= gain
    return blk


def _state(blk):
    return {k: v.detach().cpu() for k, v in blk.state_dict().items()}


def _rel(a, b):
    return C.rel_l2(a.detach().cpu(), b.detach().cpu())


# fc_gamma.2.bias: a per-channel shift of the logits cancels in the softmax, its gradient (the column sums of dL) is 0 up to
# rounding in every precision and has no relative error.  It is bounded by the size of the terms that cancel in it instead:
# 1e-6 x the largest column sum of |dL| (fp64 restatement); the kernel test of these column sums measures 1e-7.
_ZERO_GRAD = 'fc_gamma.2.bias'


def _assert_zero_grad_is_rounding(grad, dL, what):
    bar = 1e-6 * float(dL.abs().reshape(-1, dL.shape[-1]).sum(0).max())
    worst = float(grad.detach().abs().max())
    print('%-20s max |grad| %.3e, 1e-6 x sum of |dL| terms %.3e (%s)' % (_ZERO_GRAD, worst, bar, what))
    assert worst <= bar, (what, worst, bar)


@pytest.mark.parametrize('gain', [256.0, 1024.0])
@pytest.mark.parametrize('B,n,dp', [(2, 37, 64), (3, 16, 128)])
def test_fused_attention_fp32_against_fp64_in_the_peaked_regime(B, n, dp, gain):
    """D1: outputs, d feat and every parameter gradient of the fused fp32 path are as close to fp64 (relative L2) as
    4 x the GPU fp32 composition's own error; no absolute term."""
    blk = _gained_block(dp, 1, gain)
    g = torch.Generator().manual_seed(n)
    xyz = torch.rand(B, n, 3, generator=g)
    feat = torch.randn(B, n, dp, generator=g)
    probe = torch.randn(B, n, dp, generator=g)
    o1, gf1, gr1 = _run(blk, xyz.cuda(), feat.cuda(), probe.cuda(), True)
    o0, gf0, gr0 = _run(blk, xyz.cuda(), feat.cuda(), probe.cuda(), False)
    nbr = blk.neighbours(xyz.cuda()).cpu()
    ro, rgf, rmid, rgr = C.block_grads(_state(blk), xyz, feat, nbr, probe)
    _assert_zero_grad_is_rounding(gr1[_ZERO_GRAD], rmid['dL'], 'fused')
    _assert_zero_grad_is_rounding(gr0[_ZERO_GRAD], rmid['dL'], 'composition')
    a = C.block_forward(_state(blk), xyz, feat, nbr)[1]['attn']
    print('gain %g: softmax weights %.1e .. %.3f' % (gain, float(a.min()), float(a.max())))
    assert float(a.max()) > 0.5
    rows = [('out', o1, o0, ro), ('dfeat', gf1, gf0, rgf)] + [(k, gr1[k], gr0[k], rgr[k]) for k in sorted(gr0) if k != _ZERO_GRAD]
    bad = []
    for name, fused, comp, ref in rows:
        e1, e0 = _rel(fused, ref), _rel(comp, ref)
        print('%-20s rel L2 vs fp64: fused %.3e  composition %.3e  ratio %.2f' % (name, e1, e0, e1 / e0))
        if not e1 <= 4 * e0:
            bad.append((name, e1, e0))
    assert not bad, bad


@pytest.mark.parametrize('gain', [256.0, 1024.0])
@pytest.mark.parametrize('B,n', [(2, 64), (3, 16)])
def test_one_kernel_fp16_forward_against_fp64_in_the_peaked_regime(B, n, gain):
    """D2: sug_ptran_fused_fwd's mixed and every tensor it saves for the backward, against fp64: at most 2 x the error of the
    composed fp16 chain, which rounds at the same points (the factor covers another order of the GEMMs' partial sums)."""
    from sug_amd import ops
    blk = _gained_block(64, 3, gain)
    g = torch.Generator().manual_seed(B * 1000 + n)
    xyz = torch.rand(B, n, 3, generator=g)
    feat = torch.randn(B, n, 64, generator=g)
    nbr = blk.neighbours(xyz.cuda())
    mid = C.block_forward(_state(blk), xyz, feat, nbr.cpu())[1]
    q, kf, vf = (mid[t].float().cuda().requires_grad_(True) for t in ('q', 'kf', 'vf'))
    st = _state(blk)                      # the reference restarts from the fp32 q / K / V that the kernels are given
    P = {k: v.double() for k, v in st.items()}
    delta = C.pos1(xyz, nbr.cpu(), P['fc_delta.0.weight'], P['fc_delta.0.bias']) @ P['fc_delta.2.weight'].t() + P['fc_delta.2.bias']
    U = C.qk(q.detach().cpu(), kf.detach().cpu(), delta, nbr.cpu())
    T1 = torch.relu(U @ P['fc_gamma.0.weight'].t() + P['fc_gamma.0.bias'])
    Lg = T1 @ P['fc_gamma.2.weight'].t() + P['fc_gamma.2.bias']
    mixed, mx, sm, _ = C.attn(Lg, delta, vf.detach().cpu(), nbr.cpu())
    want = {'mixed': mixed, 'T0': C.pos1(xyz, nbr.cpu(), P['fc_delta.0.weight'], P['fc_delta.0.bias']), 'delta': delta, 'U': U,
            'T1': T1, 'L': Lg, 'mx': mx, 'sm': sm}
    got, keep = {}, ops.PTRAN_FUSED
    try:
        for fused in (True, False):
            ops.PTRAN_FUSED = fused
            out = ops.ptran_attention(xyz.cuda(), nbr, q, kf, vf, blk.fc_delta, blk.fc_gamma, torch.float16)
            s = out.grad_fn.saved_tensors          # xyz, nbr, vf, w1, b1, w2, wg1, wg2, T0, delta, U, T1, L, mx, sm, mixed
            got[fused] = dict(zip(('T0', 'delta', 'U', 'T1', 'L', 'mx', 'sm', 'mixed'), s[8:16]))
    finally:
        ops.PTRAN_FUSED = keep
    bad = []
    for name in ('mixed', 'T0', 'delta', 'U', 'T1', 'L', 'mx', 'sm'):
        shape = want[name].shape
        e1, e0 = _rel(got[True][name].view(shape), want[name]), _rel(got[False][name].view(shape), want[name])
        print('%-6s rel L2 vs fp64: one kernel %.3e  composed fp16 chain %.3e' % (name, e1, e0))
        if not e1 <= 2 * e0 + 1e-7:
            bad.append((name, e1, e0))
    assert not bad, bad


# ----------------------------------------------------------------------------- gradients at a real loss's scale
# The backward is linear in the incoming gradient g: for s a power of two the exact gradients of s * probe are s times
# those of probe, and arithmetic that keeps fp32 (or properly scaled fp16) values reproduces that.  An O(1) probe leaves
# the k-expanded fp16 gradients at O(1e-2); under a mean-reduced loss they are 2^-20 of that and below fp16's normals.
_SCALES = (1.0, 2.0 ** -12, 2.0 ** -20)


@functools.lru_cache(maxsize=None)
def _scale_case(gain):
    blk = _gained_block(64, 1, gain)
    B, n = 2, 64
    g = torch.Generator().manual_seed(64)
    xyz = torch.rand(B, n, 3, generator=g)
    feat = torch.randn(B, n, 64, generator=g)
    probe = torch.randn(B, n, 64, generator=g)
    gm = torch.randn(B, n, 512, generator=g)
    nbr = blk.neighbours(xyz.cuda()).cpu()
    st = _state(blk)
    mid = C.block_forward(st, xyz, feat, nbr)[1]
    q, kf, vf = (mid[t].float() for t in ('q', 'kf', 'vf'))
    att = {k: v for k, v in st.items() if k.startswith(('fc_delta', 'fc_gamma'))}
    _, aqkv, apar = C.attention_grads(att, xyz, nbr, q, kf, vf, gm)
    _, bgf, bmid, bpar = C.block_grads(st, xyz, feat, nbr, probe)
    adL = aqkv.pop('dL')
    return dict(blk=blk, xyz=xyz, feat=feat, probe=probe, gm=gm, nbr=nbr, q=q, kf=kf, vf=vf,
                ref_attn={**aqkv, **apar}, ref_block={'dfeat': bgf, **bpar}, dL_attn=adL, dL_block=bmid['dL'])


def _assert_scale_invariant(results, ref, fp32, dL):
    """results: {s: {name: gradient / s}}.  Every gradient finite (an fp16 overflow of the scaled backward would show as
    inf / nan here).  fp32: the same bits at every s.  fp16: the relative L2 error against fp64 at each s at most 2 x that at
    s = 1, + 1e-7 (ideal scaled arithmetic is exactly invariant: the factor is a condition, with room for fp32 subnormals at
    the small end and nothing else)."""
    names = [k for k in sorted(ref) if k != _ZERO_GRAD]
    for s in _SCALES:
        for k, v in results[s].items():
            assert bool(torch.isfinite(v).all()), '%s is not finite at s = %g' % (k, s)
        _assert_zero_grad_is_rounding(results[s][_ZERO_GRAD], dL, 's = %g' % s)
    bad = []
    for k in names:
        errs = [_rel(results[s][k], ref[k]) for s in _SCALES]
        print('%-20s rel L2 vs fp64 at s = 1, 2^-12, 2^-20: %s' % (k, '  '.join('%.3e' % e for e in errs)))
        if fp32:
            if not all(torch.equal(results[s][k], results[1.0][k]) for s in _SCALES):
                bad.append((k, 'bits differ', errs))
        elif not all(e <= 2 * errs[0] + 1e-7 for e in errs):
            bad.append((k, errs))
    if fp32:
        assert all(torch.equal(results[s][_ZERO_GRAD], results[1.0][_ZERO_GRAD]) for s in _SCALES if _ZERO_GRAD in results[s])
    assert not bad, bad


# gain 1024: softmax weights up to 1.0 and the largest fc_gamma[2] rows -- where the scaled fp16 GEMM results (dT1, dU, dT0)
# are largest: the headroom stated above ops._G16_LOG2_TARGET
@pytest.mark.parametrize('gain', [1.0, 256.0, 1024.0])
@pytest.mark.parametrize('mode', ['fp32', 'fp16'])
def test_attention_gradients_scale_with_the_incoming_gradient(mode, gain):
    from sug_amd import ops
    c = _scale_case(gain)
    blk = c['blk']
    params = {k: p for k, p in blk.named_parameters() if k.startswith(('fc_delta', 'fc_gamma'))}
    results = {}
    for s in _SCALES:
        q, kf, vf = (c[t].cuda().requires_grad_(True) for t in ('q', 'kf', 'vf'))
        mixed = ops.ptran_attention(c['xyz'].cuda(), c['nbr'].cuda(), q, kf, vf, blk.fc_delta, blk.fc_gamma,
                                    None if mode == 'fp32' else torch.float16)
        names = ['dq', 'dK', 'dV'] + sorted(params)
        grads = torch.autograd.grad(mixed, [q, kf, vf] + [params[k] for k in sorted(params)], c['gm'].cuda() * s)
        results[s] = {k: v / s for k, v in zip(names, grads)}
    _assert_scale_invariant(results, c['ref_attn'], mode == 'fp32', c['dL_attn'])


@pytest.mark.parametrize('gain', [1.0, 256.0, 1024.0])
@pytest.mark.parametrize('mode', ['fp32', 'fp16', 'fp16-proj16'])
def test_block_gradients_scale_with_the_incoming_gradient(mode, gain):
    from sug_amd.model import Ptran_transformer as PT
    c = _scale_case(gain)
    blk = c['blk']
    keep = PT.GEMM_DTYPE, PT.PROJ_16BIT
    results = {}
    try:
        PT.GEMM_DTYPE, PT.PROJ_16BIT = (None if mode == 'fp32' else torch.float16), mode == 'fp16-proj16'
        for s in _SCALES:
            _, gf, gr = _run(blk, c['xyz'].cuda(), c['feat'].cuda(), c['probe'].cuda() * s, True)
            results[s] = {'dfeat': gf / s, **{k: v / s for k, v in gr.items()}}
    finally:
        PT.GEMM_DTYPE, PT.PROJ_16BIT = keep
    _assert_scale_invariant(results, c['ref_block'], mode == 'fp32', c['dL_block'])
