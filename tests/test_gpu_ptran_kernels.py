"""Every C entry point of the Point Transformer attention (csrc/ptran.hip) against plain fp64 restatements of the same
operation (tests/ptran_kernel_cases.py), through the C ABI: dtype code 0 (fp32) and 1 (fp16 k-expanded tensors), the
shapes, neighbour-list kinds and logit regimes of that module.

Bars.  fp32 outputs: element-wise within 1e-4 of the tensor's max, and a relative L2 error against fp64 of at most
4 x that of the same restatement evaluated in plain torch fp32 (+ 1e-7 for results that are exact in both).  fp16
outputs: |got - ref| <= 2^-10 |ref| + 2^-24.  With dtype 1 the fp64 reference is evaluated on the fp16-rounded inputs
upcast exactly, so only the kernel's own arithmetic and its output rounding are under test.  Every output buffer is
NaN before the call and NaN-free after it; two calls give the same bits."""
import functools

import pytest
import torch

import ptran_kernel_cases as C

pytestmark = pytest.mark.gpu

D = C.D
F32, F64 = torch.float32, torch.float64

# (shape, list kind): every shape, every kind at a shape with k % 4 != 0
ROW_CASES = [((1, 1, 1), 'knn'), ((2, 5, 4), 'random'), ((3, 16, 16), 'knn'), ((2, 37, 15), 'knn'), ((2, 37, 15), 'random'),
             ((2, 37, 15), 'hub'), ((2, 37, 15), 'padded'), ((2, 64, 7), 'hub'), ((2, 64, 7), 'padded'), ((1, 300, 16), 'hub'),
             ((1, 300, 16), 'padded')]
# (shape, list kind, regime): every regime and every kind at a shape with k % 4 != 0; k = 1 is regime (e)
ATTN_CASES = [((1, 1, 1), 'knn', 'uniform'), ((1, 1, 1), 'knn', 'peaked'), ((2, 5, 4), 'random', 'saturated'),
              ((3, 16, 16), 'knn', 'peaked'), ((3, 16, 16), 'random', 'equal_neg'), ((2, 37, 15), 'knn', 'uniform'),
              ((2, 37, 15), 'random', 'peaked'), ((2, 37, 15), 'hub', 'saturated'), ((2, 37, 15), 'padded', 'equal_pos'),
              ((2, 37, 15), 'hub', 'equal_neg'), ((2, 64, 7), 'padded', 'peaked'), ((2, 64, 7), 'hub', 'uniform'),
              ((2, 64, 7), 'knn', 'saturated'), ((1, 300, 16), 'hub', 'peaked'), ((1, 300, 16), 'knn', 'saturated'),
              ((1, 300, 16), 'padded', 'equal_pos')]
_id = lambda c: '-'.join('x'.join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)
rows_cases = pytest.mark.parametrize('case', ROW_CASES, ids=_id)
attn_cases = pytest.mark.parametrize('case', ATTN_CASES, ids=_id)
codes = pytest.mark.parametrize('code', [0, 1], ids=['fp32', 'fp16'])


def _lo(code):
    return F32 if code == 0 else torch.float16


def _nan(shape, dtype=F32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def _call(name, *args):
    from sug_amd import ops
    conv = [ops._p(a) if isinstance(a, torch.Tensor) else a for a in args]
    ops.check(getattr(ops.lib(), name)(*conv, ops._st()), name)


def _cws(R):
    from sug_amd import ops
    return torch.empty(ops.lib().sug_ptran_colsum_workspace(R), dtype=F32, device='cuda')


def _no_nan(**outs):
    for k, v in outs.items():
        assert not bool(torch.isnan(v).any()), '%s: NaN left (an element the kernel did not write)' % k


def _fp32_bars(name, got, ref, base, scale=None, extra=0.0):
    """got: the kernel's fp32 result, ref: fp64, base: the same restatement in plain torch fp32.  extra: a term of the
    L2 bar that the caller derives from the kernel's code where the factor 4 cannot hold (see _EXP_FORM)."""
    got, ref, base = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1), base.detach().double().reshape(-1)
    assert got.shape == ref.shape
    tmax = float(ref.abs().max()) if scale is None else scale
    worst = float((got - ref).abs().max())
    ek, eb = C.rel_l2(got, ref), C.rel_l2(base, ref)
    print('%-8s max|err| %.3e (tensor max %.3e)  rel L2: kernel %.3e  torch fp32 %.3e  ratio %.2f'
          % (name, worst, tmax, ek, eb, ek / (eb + 1e-7)))
    assert worst <= 1e-4 * tmax, '%s: element-wise %.3e > 1e-4 * %.3e' % (name, worst, tmax)
    if float(ref.norm()) > 0:
        assert ek <= 4 * eb + 1e-7 + extra, '%s: relative L2 %.3e > 4 * %.3e + 1e-7 + %.1e' % (name, ek, eb, extra)


def _fp16_bar(name, got, ref):
    assert got.dtype == torch.float16
    ok, worst = C.within_fp16_ulp(got.detach().cpu(), ref.detach())
    print('%-8s fp16 output: worst |err| / (2^-10 |ref| + 2^-24) = %.3f' % (name, worst))
    assert ok, '%s: %.3f x the fp16 bar' % (name, worst)


def _out_bars(code, name, got, ref, base, scale=None, extra=0.0):
    """A k-expanded output: fp32 bars with dtype 0, the fp16 bar with dtype 1."""
    if code == 0:
        _fp32_bars(name, got, ref, base, scale, extra)
    else:
        _fp16_bar(name, got, ref)


@functools.lru_cache(maxsize=None)
def _lists(case2):
    """(xyz, nbr) on the CPU and on the GPU, reverse lists from ops.knn_reverse."""
    from sug_amd import ops
    (B, n, k), kind = case2
    xyz, nbr = C.neighbours(kind, B, n, k)
    off, ent = ops.knn_reverse(nbr.cuda())
    return xyz, nbr, xyz.cuda(), nbr.cuda(), off, ent


@rows_cases
def test_reverse_lists_match_a_numpy_construction(case):
    (B, n, k), kind = case
    _, nbr, _, _, off, ent = _lists(case)
    roff, rent = C.reverse_lists(nbr)
    assert off.shape == (B, n + 1) and ent.shape == (B, n * k)
    assert torch.equal(off.cpu(), torch.from_numpy(roff)) and torch.equal(ent.cpu(), torch.from_numpy(rent))


# ----------------------------------------------------------------------------- pos1
@codes
@rows_cases
def test_pos1_fwd_against_fp64(case, code):
    (B, n, k), kind = case
    xyz, nbr, xyz_d, nbr_d, _, _ = _lists(case)
    # fp16: dyadic inputs, W1 . rel + b1 exact in fp32.  Near a zero of the pre-activation the three fp32 roundings of its
    # O(1) terms (3 * 2^-24) exceed the bar's 2^-24, which is an fp16 ulp around the fp64 result; the fp32 arithmetic is
    # what the dtype-0 cases hold to the fp32 bars, on generic inputs
    w1, b1 = C.pos1_inputs(B, n, code == 1)
    if code == 1:
        xyz = C.dyadic_xyz(xyz)
        xyz_d = xyz.cuda()
    outs = []
    for _ in range(2):
        T0 = _nan((B, n, k, D), _lo(code))
        _call('sug_ptran_pos1_fwd', xyz_d, nbr_d, w1.cuda(), b1.cuda(), B, n, k, D, code, T0)
        outs.append(T0)
    _no_nan(T0=outs[0])
    assert torch.equal(outs[0], outs[1])
    ref, base = C.pos1(xyz, nbr, w1, b1), C.pos1(xyz, nbr, w1, b1, F32)
    _out_bars(code, 'T0', outs[0], ref, base)
    if kind == 'padded' and n // 3:          # a copy of point 0 named by point 0 (and the reverse): rel = 0, T0 = relu(b1) exactly
        both = (nbr >= n - n // 3) & (torch.arange(n)[None, :, None] >= n - n // 3)
        if bool(both.any()):
            assert torch.equal(outs[0].cpu()[both], torch.relu(b1).to(_lo(code)).expand(int(both.sum()), D))


@codes
@rows_cases
def test_pos1_bwd_against_fp64(case, code):
    (B, n, k), kind = case
    xyz, nbr, _, nbr_d, _, _ = _lists(case)
    xyz = C.dyadic_xyz(xyz)                  # W1 . rel + b1 exact in fp32: the ReLU mask is the reference's
    w1, b1 = C.pos1_inputs(B, n, True)
    g = torch.randn(B, n, k, D, generator=C.gen('pos1_g', case)).to(_lo(code))
    outs = []
    for _ in range(2):
        dw1, db1, ws = _nan((D, 3)), _nan((D,)), torch.empty(1024 * 4 * D, dtype=F32, device='cuda')
        _call('sug_ptran_pos1_bwd', g.cuda(), xyz.cuda(), nbr_d, w1.cuda(), b1.cuda(), B, n, k, D, code, dw1, db1, ws)
        outs.append((dw1, db1))
    _no_nan(dW1=outs[0][0], db1=outs[0][1])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref, base = C.pos1_grads(g.float(), xyz, nbr, w1, b1), C.pos1_grads(g.float(), xyz, nbr, w1, b1, F32)
    _fp32_bars('dW1', outs[0][0], ref[0], base[0])
    _fp32_bars('db1', outs[0][1], ref[1], base[1])


# ----------------------------------------------------------------------------- qk
@codes
@rows_cases
def test_qk_fwd_against_fp64(case, code):
    (B, n, k), kind = case
    _, nbr, _, nbr_d, _, _ = _lists(case)
    q, kf, delta = C.qk_inputs(B, n, k, _lo(code))
    outs = []
    for _ in range(2):
        U = _nan((B, n, k, D), _lo(code))
        _call('sug_ptran_qk_fwd', q.cuda(), kf.cuda(), delta.cuda(), nbr_d, B, n, k, D, code, U)
        outs.append(U)
    _no_nan(U=outs[0])
    assert torch.equal(outs[0], outs[1])
    _out_bars(code, 'U', outs[0], C.qk(q, kf, delta.float(), nbr), C.qk(q, kf, delta.float(), nbr, F32))


@codes
@rows_cases
def test_qk_bwd_and_its_reverse_sum_against_fp64(case, code):
    (B, n, k), kind = case
    _, nbr, _, nbr_d, off, ent = _lists(case)
    g = C.gen('qk_bwd', case)
    dU = torch.randn(B, n, k, D, generator=g).to(_lo(code))
    da = torch.randn(B, n, k, D, generator=g).to(_lo(code))
    outs = []
    for _ in range(2):
        dd, dq, dk, db = da.cuda().clone(), _nan((B, n, D)), _nan((B, n, D)), _nan((D,))
        _call('sug_ptran_qk_bwd', dU.cuda(), dd, off, ent, B, n, k, D, code, dq, dk, db, _cws(B * n * k))
        outs.append((dd, dq, dk, db))
    _no_nan(ddelta=outs[0][0], dq=outs[0][1], dK=outs[0][2], db=outs[0][3])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    ref, base = C.qk_grads(dU.float(), da.float(), nbr, B, n), C.qk_grads(dU.float(), da.float(), nbr, B, n, F32)
    dd, dq, dk, db = outs[0]
    _out_bars(code, 'd delta', dd, ref[2], base[2])
    _fp32_bars('dq', dq, ref[0], base[0])
    _fp32_bars('dK', dk, ref[1], base[1])
    _fp32_bars('db2', db, ref[3], base[3])
    if kind == 'hub' and C.orphans(n):
        assert float(dk.cpu()[:, C.orphans(n)].abs().max()) == 0.0, 'orphans: dK rows are exactly 0'
    # db2 = None: the column sums are optional, the rest is the same
    dd2, dq2, dk2 = da.cuda().clone(), _nan((B, n, D)), _nan((B, n, D))
    _call('sug_ptran_qk_bwd', dU.cuda(), dd2, off, ent, B, n, k, D, code, dq2, dk2, None, None)
    assert torch.equal(dd2, dd) and torch.equal(dq2, dq) and torch.equal(dk2, dk)


# ----------------------------------------------------------------------------- ReLU mask
@codes
@rows_cases
def test_relu_bwd_db_against_fp64(case, code):
    (B, n, k), kind = case
    g = C.gen('relu', case)
    G = torch.randn(B * n * k, D, generator=g).to(_lo(code))
    T1 = torch.relu(torch.randn(B * n * k, D, generator=g)).to(_lo(code))       # exact zeros, as a ReLU leaves them
    outs = []
    for _ in range(2):
        Gd, db = G.cuda().clone(), _nan((D,))
        _call('sug_ptran_relu_bwd_db', Gd, T1.cuda(), B * n * k, D, code, db, _cws(B * n * k))
        outs.append((Gd, db))
    _no_nan(G=outs[0][0], db=outs[0][1])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref, base = C.relu_mask(G.float(), T1.float()), C.relu_mask(G.float(), T1.float(), F32)
    assert torch.equal(outs[0][0].cpu().double(), ref[0]), 'the masked gradient is exact'
    _fp32_bars('dbg1', outs[0][1], ref[1], base[1])


# ----------------------------------------------------------------------------- attention
# _EXP_FORM.  Where the factor 4 against plain torch fp32 cannot hold, from the kernels' code: the exponentials are
# exp2(fma(l, scale * log2e, -max * log2e)) with max = fl(l_max * scale).  For the largest logit the argument is not 0 but the
# rounding of the three constants of that fma, r <= 3 * 2^-24 * |l * scale| * log2e, so that every exponential of a (point,
# channel) carries the common factor 2^r where plain exp(z - max) has exactly 1 for the maximum.  The factor cancels in
# mixed, and in the weights the backward rebuilds (same form, same saved sum), but it stays in the saved sum itself:
#   sm    relative error up to ln2 * r = 3 * 2^-24 * max|l * scale|   (8.8e-5 measured at |l * scale| = 885, regime (c))
#   da, dL   the rebuilt weight e * (1 / sum) has two fp32 roundings (2^-23) where e / sum with e = 1 and sum = 16 has none
# These two terms are added to the L2 bar of those tensors only; the element-wise bar of 1e-4 stays as it is.
def _sm_extra(L):
    return 3 * 2.0 ** -24 * float((L.double() * C.SCALE).abs().max())


_PR_EXTRA = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _attn_case(case, code):
    """Inputs (rounded to the dtype), the kernel's forward and backward (two calls each), the fp64 and fp32 restatements."""
    (B, n, k), kind, regime = case
    xyz, nbr, _, nbr_d, off, ent = _lists((case[0], kind))
    lo = _lo(code)
    L = C.logits(regime, B, n, k).to(lo)
    delta, vf, g = C.attn_inputs(B, n, k, lo)
    Ld, dd, vd, gd = L.cuda(), delta.cuda(), vf.cuda(), g.cuda()
    fwd, bwd = [], []
    for _ in range(2):
        mixed, mx, sm = _nan((B, n, D)), _nan((B, n, D)), _nan((B, n, D))
        _call('sug_ptran_attn_fwd', Ld, dd, vd, nbr_d, B, n, k, D, code, C.SCALE, mixed, mx, sm)
        fwd.append((mixed, mx, sm))
        dL, da, dv, db = _nan((B, n, k, D), lo), _nan((B, n, k, D), lo), _nan((B, n, D)), _nan((D,))
        _call('sug_ptran_attn_bwd', gd, mixed, Ld, dd, vd, nbr_d, mx, sm, off, ent, B, n, k, D, code, C.SCALE, dL, da, dv, db,
              _cws(B * n * k))
        bwd.append((dL, da, dv, db))
    Lf, df = L.float(), delta.float()
    ref = C.attn(Lf, df, vf, nbr)[:3] + C.attn_grads(g, Lf, df, vf, nbr)
    base = C.attn(Lf, df, vf, nbr, F32)[:3] + C.attn_grads(g, Lf, df, vf, nbr, F32)
    return dict(L=Lf, delta=df, vf=vf, g=g, nbr=nbr, fwd=fwd, bwd=bwd, ref=ref, base=base)


@codes
@attn_cases
def test_attn_fwd_against_fp64(case, code):
    (B, n, k), kind, regime = case
    c = _attn_case(case, code)
    (mixed, mx, sm), again = c['fwd']
    _no_nan(mixed=mixed, mx=mx, sm=sm)
    for a, b in zip(c['fwd'][0], again):
        assert torch.equal(a, b)
    for name, got, r, b in zip(('mixed', 'mx', 'sm'), (mixed, mx, sm), c['ref'], c['base']):
        _fp32_bars(name, got, r, b, extra=_sm_extra(c['L']) if name == 'sm' else 0.0)
    y = C.gather(c['vf'], c['nbr']) + c['delta']                       # fp32, as the kernel adds them
    if regime in ('equal_pos', 'equal_neg'):        # the max subtraction alone: the plain mean
        mean64 = (C.gather(c['vf'].double(), c['nbr']) + c['delta'].double()).mean(2)
        _fp32_bars('mean', mixed, mean64, y.mean(2))


@codes
@pytest.mark.parametrize('case', [c for c in ATTN_CASES if c[2] == 'saturated' or c[0][2] == 1], ids=_id)
def test_attn_fwd_one_hot_softmax_returns_the_selected_row_bit_for_bit(case, code):
    """Regime (c), and k = 1: the weights are exactly one-hot, so mixed is the selected neighbour's fl(V + delta)."""
    (B, n, k), kind, regime = case
    c = _attn_case(case, code)
    mixed = c['fwd'][0][0].cpu()
    y = C.gather(c['vf'], c['nbr']) + c['delta']                       # fp32, as the kernel adds them
    want = y.gather(2, C.selected(c['L']))[:, :, 0]
    diff = mixed != want
    ulp = float(((mixed - want).abs() / want.abs().clamp_min(1e-30)).max())
    print('one-hot: %d of %d elements differ, largest relative difference %.3e' % (int(diff.sum()), diff.numel(), ulp))
    assert torch.equal(mixed, want)


@codes
@attn_cases
def test_attn_bwd_and_its_reverse_sum_against_fp64(case, code):
    (B, n, k), kind, regime = case
    c = _attn_case(case, code)
    (dL, da, dv, db), again = c['bwd']
    _no_nan(dL=dL, da=da, dV=dv, dbg2=db)
    for a, b in zip(c['bwd'][0], again):
        assert torch.equal(a, b)
    rdL, rda, rdv, rdb = c['ref'][3:]
    bdL, bda, bdv, bdb = c['base'][3:]
    gy = float((c['g'].double()[:, :, None] * (C.gather(c['vf'].double(), c['nbr']) + c['delta'].double())).abs().max())
    _out_bars(code, 'da', da, rda, bda, extra=_PR_EXTRA)
    exact_zero = regime == 'saturated' or k == 1        # one-hot weights: dL = 0, no tensor max to refer to
    if exact_zero:
        worst = float(dL.float().abs().max())
        print('dL       max |dL| %.3e   1e-6 * max|g.y| = %.3e' % (worst, 1e-6 * gy))
        assert float(rdL.abs().max()) <= 1e-12 * gy
        assert worst <= 1e-6 * gy
        if k == 1:
            assert worst == 0.0, 'k = 1: dL is exactly 0'
    else:
        _out_bars(code, 'dL', dL, rdL, bdL, extra=_PR_EXTRA)
    if regime in ('equal_pos', 'equal_neg') and code == 0:
        # uniform weights: dL_j = g (y_j - mean y) / (k sqrt(d)) is not 0 (the y_j differ), its sum over the neighbours is
        worst = float(dL.sum(2).abs().max())
        print('sum_j dL max %.3e   1e-6 * max|g.y| = %.3e' % (worst, 1e-6 * gy))
        assert worst <= 1e-6 * gy
    # dV: over the reverse lists of the da the kernel stored (fp16 with dtype 1), and with dtype 0 also end to end
    v0 = torch.zeros(B, n, D, dtype=F64, requires_grad=True)
    (sum64,) = torch.autograd.grad((C.gather(v0, c['nbr']) * da.cpu().double()).sum(), v0)
    v1 = torch.zeros(B, n, D, dtype=F32, requires_grad=True)
    (sum32,) = torch.autograd.grad((C.gather(v1, c['nbr']) * da.cpu().float()).sum(), v1)
    _fp32_bars('dV(sum)', dv, sum64, sum32)
    if code == 0:
        _fp32_bars('dV', dv, rdv, bdv)
    if kind == 'hub' and C.orphans(n):
        assert float(dv.cpu()[:, C.orphans(n)].abs().max()) == 0.0, 'orphans: dV rows are exactly 0'
    # column sums of dL: softmax gradients sum to 0 over the neighbours, so the tensor is 0 up to rounding and has no max
    # of its own; the scale of the sum is that of its terms, max over the channels of sum_r |dL|
    # (where dL itself is 0 up to rounding: the element bar above, 1e-6 max|g.y|, times the number of rows)
    bar = 1e-6 * gy * B * n * k if exact_zero else 1e-4 * float(rdL.abs().reshape(-1, D).sum(0).max())
    err = float((db.cpu().double() - rdb).abs().max())
    print('dbg2     max|err| %.3e   bar %.3e' % (err, bar))
    assert err <= bar


# ----------------------------------------------------------------------------- range scaling of the fp16 backward
@pytest.mark.parametrize('sizes,peak', [((1,), 1.0), ((4095,), 3e-6), ((5, 1 << 20, 77), 0.999), ((1 << 21,), 16.0), ((4097, 3), 15.9),
                                        ((64,), 0.0), ((1000,), 3e-39), ((1000,), float('inf')), ((2049, 2049, 2049), 1e30)])
def test_grad_scale16_is_the_power_of_two_of_the_largest_magnitude(sizes, peak):
    """sug_grad_scale16 against its definition: s * max|g| in [2^(t-1), 2^t), s a power of two clamped to 2^+-100, and
    out[1] = 1 / s exactly; odd sizes (scalar tail), several workgroups, a pointer that is not 16-byte aligned."""
    import math
    from sug_amd import ops
    t = ops._G16_LOG2_TARGET
    g = C.gen('scale', sizes, peak)
    hosts = [torch.randn(n + 1, generator=g).clamp_(-1, 1) * (peak if math.isfinite(peak) else 1.0) * 0.5 for n in sizes]
    where = len(sizes) - 1
    hosts[where][sizes[where] // 2 + 1] = -peak                     # the maximum, negative, in the last tensor
    devs = [h.cuda()[1:] for h in hosts]                             # offset by one float: not 16-byte aligned
    assert devs[0].data_ptr() % 16 == 4
    s, inv = ops._grad_scale16(*devs)
    s2, inv2 = ops._grad_scale16(*[d.clone() for d in devs])         # aligned copies
    assert float(s) == float(s2) and float(inv) == float(inv2)
    m = max(float(h[1:].double().abs().max()) for h in hosts)
    if m == 0 or m < 2.0 ** -126:
        e = 100
    elif math.isinf(m):
        e = -100
    else:
        e = max(-100, min(100, t - 1 - math.floor(math.log2(m))))
    assert float(s) == 2.0 ** e and float(inv) == 2.0 ** -e, (float(s), e)
    if 0 < m < float('inf') and abs(e) < 100:
        assert 2.0 ** (t - 1) <= float(s) * m < 2.0 ** t


# ----------------------------------------------------------------------------- fp16 outputs at full magnitude
# The fp16 cases above size their inputs so that fp32 cancellation fits inside the one-ulp bar.  Here the inputs are the
# fp32 cases' (|V + delta| up to ~10, |g| up to ~4.5, generic W1 / b1 / xyz), and the bar carries the cancellation term
# explicitly: the fp32 roundings of the terms that cancel, counted from the kernel's code, each at most 2^-24 of its term.
def _fp16_bar_with(name, got, ref, term):
    """|got - ref| <= 2^-10 |ref| + 2^-24 + term (element-wise or scalar)."""
    ref = ref.detach().double()
    err = (got.detach().cpu().double() - ref).abs()
    bar = ref.abs() * 2.0 ** -10 + 2.0 ** -24 + term
    plain = ref.abs() * 2.0 ** -10 + 2.0 ** -24
    print('%-8s fp16 output at full magnitude: worst |err| / bar = %.3f (against the plain one-ulp bar: %.3f)'
          % (name, float((err / bar).max()), float((err / plain).max())))
    assert bool((err <= bar).all()), name


@pytest.mark.parametrize('case', [((2, 37, 15), 'knn'), ((1, 300, 16), 'padded')], ids=_id)
def test_pos1_fwd_fp16_on_generic_inputs(case):
    """t = fma(wz, ez, fma(wy, ey, wx * ex)) + b1: four roundings (product, two fmas, sum), each at most 2^-24 of a partial sum
    that is at most |wx ex| + |wy ey| + |wz ez| + |b1|; the differences ex, ey, ez carry one rounding of their own."""
    (B, n, k), kind = case
    xyz, nbr, xyz_d, nbr_d, _, _ = _lists(case)
    w1, b1 = C.pos1_inputs(B, n, False)
    T0 = _nan((B, n, k, D), torch.float16)
    _call('sug_ptran_pos1_fwd', xyz_d, nbr_d, w1.cuda(), b1.cuda(), B, n, k, D, 1, T0)
    _no_nan(T0=T0)
    rel = (xyz.double()[:, :, None] - C.gather(xyz.double(), nbr)).abs()
    size = rel @ w1.double().abs().t() + b1.double().abs()
    _fp16_bar_with('T0', T0, C.pos1(xyz, nbr, w1, b1), 5 * 2.0 ** -24 * size)


@pytest.mark.parametrize('case', [((2, 37, 15), 'random', 'peaked'), ((1, 300, 16), 'hub', 'peaked'), ((2, 37, 15), 'hub', 'saturated')],
                         ids=_id)
def test_attn_bwd_fp16_at_full_magnitude(case):
    """dL = a (g y - g mixed) / sqrt(d) for the winning neighbour of a peaked softmax is the difference of two fp32 products
    of size |g y|: y = V + delta (1 rounding), g y (1), mixed (the forward's k fmas and its division, as stored: 4), g mixed
    (1), the difference (1): 8 roundings of at most 2^-24 max|g y| each, times a <= 1 and 1 / sqrt(d).  da = g a has no
    cancellation and keeps the plain bar; in the saturated regime |V + delta| ~ 10 and a = 1: da = g exactly, dL = 0."""
    (B, n, k), kind, regime = case
    xyz, nbr, _, nbr_d, off, ent = _lists((case[0], kind))
    L = C.logits(regime, B, n, k).half()
    delta, vf, g = C.attn_inputs(B, n, k)                     # the fp32 cases' magnitudes
    delta = delta.half()
    Ld, dd, vd, gd = L.cuda(), delta.cuda(), vf.cuda(), g.cuda()
    mixed, mx, sm = _nan((B, n, D)), _nan((B, n, D)), _nan((B, n, D))
    _call('sug_ptran_attn_fwd', Ld, dd, vd, nbr_d, B, n, k, D, 1, C.SCALE, mixed, mx, sm)
    dL, da, dv = _nan((B, n, k, D), torch.float16), _nan((B, n, k, D), torch.float16), _nan((B, n, D))
    _call('sug_ptran_attn_bwd', gd, mixed, Ld, dd, vd, nbr_d, mx, sm, off, ent, B, n, k, D, 1, C.SCALE, dL, da, dv, None, None)
    _no_nan(dL=dL, da=da, dV=dv)
    rdL, rda, _, _ = C.attn_grads(g, L.float(), delta.float(), vf, nbr)
    gy = float((g.double()[:, :, None] * (C.gather(vf.double(), nbr) + delta.double())).abs().max())
    print('max |g y| = %.1f, max |V + delta| = %.1f' % (gy, float((C.gather(vf, nbr) + delta.float()).abs().max())))
    assert bool(torch.isfinite(dL).all()) and bool(torch.isfinite(da).all())
    _fp16_bar('da', da, rda)
    _fp16_bar_with('dL', dL, rdL, 8 * 2.0 ** -24 * gy * C.SCALE)
