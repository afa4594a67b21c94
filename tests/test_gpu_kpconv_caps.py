"""GPU: the KPConv row layout with dead rows (sug_amd/csrc/kpconv.hip "ROW LAYOUT") -- the pyramid at
capacity against the reference's pyramid, every op on a NaN-padded buffer against itself on a tight one, the reference's
KPConv call, the models with level caps against the goldens, one hipGraph over preprocessing + forward + backward replayed on a batch of other
level sizes, SourceStep / SUGStep / eval_graphs replay against eager launches, and the overflow contract (last)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, 'tests', 'golden', 'kpconv.npz')
DEV = 'cuda'
GOLD_CAPS = (976, 656, 256, 80)                 # capacities 3904 / 2624 / 1024 / 320 for the golden batch's 3801 / 2573 / 954 / 261
NAN = float('nan')


def _gold():
    return np.load(GOLD)


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int64)).tobytes()).hexdigest()


def _model(tag='net', caps=None):
    from sug_amd.model.Model import Net_MDA
    from sug_amd.model.KPConv_model import KPFCls
    z = _gold()
    shapes = {k: tuple(int(s) for s in sh.split(',') if s) for k, sh in zip(z[tag + '_keys'], z[tag + '_shapes'])}
    sd = O.fill_params(shapes, 7)
    for k, v in zip(z[tag + '_kp_keys'], z[tag + '_kp']):
        sd[k] = torch.from_numpy(v)
    m = Net_MDA('KPConv') if tag == 'net' else KPFCls()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    if caps is not None:
        (m.g if tag == 'net' else m).set_level_caps(caps)
    return m


def _x():
    return torch.from_numpy(_gold()['x']).to(DEV)


_SYNTH = {}


def _synth():
    """(the three batches [4,3,256,1]: synthetic normalised clouds scaled by 1.0 / 0.35 / 0.6 -- level totals that move by a
    factor of up to 8 -- , the caps calibrate_level_caps measures over them, the exact-size level lengths of each)."""
    if not _SYNTH:
        from sug_amd.model.KPConv_model import calibrate_level_caps, PreprocessorGPU, KPConvConfig, _split_clouds
        g = torch.Generator().manual_seed(0)
        xs = [(O.synth_clouds(4, 256, g) * s).to(DEV) for s in (1.0, 0.35, 0.6)]
        _SYNTH['x'] = xs
        _SYNTH['caps'] = calibrate_level_caps(xs)
        _SYNTH['lengths'] = [PreprocessorGPU(KPConvConfig).forward_packed(*_split_clouds(x))['lengths'] for x in xs]
    return _SYNTH['x'], _SYNTH['caps'], _SYNTH['lengths']


def _state_hash(net):
    h = hashlib.sha256()
    for k, v in sorted(net.state_dict().items()):
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


# ----------------------------------------------------------------------------------------------- 1. the pyramid
def test_capacity_pyramid_matches_reference_pyramid():
    from sug_amd.model.KPConv_model import PreprocessorGPU, KPConvConfig, level_capacity
    z = _gold()
    x = _x()
    B, N = x.shape[0], x.shape[2]
    pts = x.squeeze(-1).permute(0, 2, 1).reshape(B * N, 3).contiguous()
    pre = PreprocessorGPU(KPConvConfig)
    pre.set_level_caps(GOLD_CAPS)
    meta = pre.forward_packed(pts, [N] * B)
    L = int(z['levels'])
    C = level_capacity(B, N, GOLD_CAPS)
    assert C == [4096, 3904, 2624, 1024, 320] and meta['capacities'] == C
    assert meta['lengths'] is None and len(meta['points']) == L
    tot = [int(z['lengths_%d' % l].sum()) for l in range(L)]

    def table(t, rows, cap_shadow, shadow):
        """The valid rows with the capacity shadow rewritten to the exact-size shadow; the dead rows are all shadow."""
        t = t.cpu().long()
        assert t.shape[0] >= rows and bool((t[rows:] == cap_shadow).all())
        v = t[:rows].clone()
        assert int(v.max()) <= cap_shadow and not bool(((v >= shadow) & (v < cap_shadow)).any())
        v[v == cap_shadow] = shadow
        return v

    for l in range(L):
        off = meta['offsets'][l].cpu().numpy()
        assert np.array_equal(np.diff(off), z['lengths_%d' % l]), l
        assert np.array_equal(meta['stack_lengths'][l].cpu().numpy(), z['lengths_%d' % l]), l
        p = meta['points'][l].cpu().numpy()
        assert p.shape == (C[l], 3)
        assert np.array_equal(p[:tot[l]], z['points_%d' % l]), l                             # bit-exact
        assert not p[tot[l]:].any(), l                                                        # dead rows: zero
        assert _sha(table(meta['neighbors'][l], tot[l], C[l], tot[l])) == str(z['neighbors_sha_%d' % l]), l
        be = meta['rev_neighbors'][l][0].cpu()
        assert be.shape == (C[l], 2) and bool((be[tot[l]:, 0] == be[tot[l]:, 1]).all()), l  # dead supports: empty lists
        if l < L - 1:
            assert _sha(table(meta['pools'][l], tot[l + 1], C[l], tot[l])) == str(z['pools_sha_%d' % l]), l
            assert _sha(table(meta['upsamples'][l], tot[l], C[l + 1], tot[l + 1])) == str(z['upsamples_sha_%d' % l]), l
    rep = pre.capacity_report()
    assert rep['overflows'] == 0
    assert [r['needed'] for r in rep['levels']] == tot[1:] and [r['capacity'] for r in rep['levels']] == C[1:]
    assert all(r['cap_needed'] <= r['cap'] for r in rep['levels'])


# ----------------------------------------------------------------------------------------------- 2. the ops
LENS, CAP = [37, 2, 60], 128


def _case(seed=0, lens=LENS, cap=CAP):
    g = torch.Generator().manual_seed(seed)
    n = sum(lens)
    pts = torch.rand(n, 3, generator=g) * 0.2
    pts[lens[0] - 1] += 5.0                                  # isolated point: only itself within the radius
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return pts.to(DEV), off.to(DEV), n, g


def _pad(t, cap=CAP, fill=NAN):
    """t [n, ...] -> [cap, ...] with the dead rows filled (NaN: reading one poisons the result)."""
    out = torch.full((cap,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def _tables(pts, off, n, r, H):
    """(tight table, tight reverse lists, padded table, padded reverse lists) of one level against itself: the n rows
    alone, and in a buffer of CAP rows whose dead rows are NaN."""
    from sug_amd import ops
    nbr = ops.radius_neighbors(pts, off, pts, off, r, H)
    rev = ops.radius_reverse(nbr, off, off, n, max(LENS))
    pc = _pad(pts)
    nbc = ops.radius_neighbors(pc, off, pc, off, r, H)
    revc = ops.radius_reverse(nbc, off, off, CAP, max(LENS))
    return nbr, rev, nbc, revc


def test_tables_and_reverse_lists_on_uneven_clouds():
    pts, off, n, _ = _case(1)
    H = 12
    nbr, (be, ent), nbc, (bec, entc) = _tables(pts, off, n, 0.08, H)
    v = nbc[:n].clone()
    assert bool((nbc[n:] == CAP).all())                     # dead queries: all shadow
    assert not bool(((v >= n) & (v < CAP)).any())
    v[v == CAP] = n
    assert torch.equal(v, nbr) and int(nbr.max()) <= n      # (the tight table's shadow is n)
    assert torch.equal(bec[:n], be)                         # the same lists at the same places
    assert bool((bec[n:, 0] == bec[n:, 1]).all())           # dead supports: empty
    be_h, ent_h, entc_h = be.cpu(), ent.cpu(), entc.cpu()
    for s in range(n):
        lo, hi = int(be_h[s, 0]), int(be_h[s, 1])
        assert torch.equal(ent_h[lo:hi], entc_h[lo:hi]), s


@pytest.mark.parametrize('Cin', [1, 16, 33])
def test_kpconv_cap_on_uneven_clouds(Cin):
    from sug_amd import ops
    pts, off, n, g = _case(Cin)
    H, K, Cout, r = 12, 15, 24, 0.08
    nbr, rev, nbc, revc = _tables(pts, off, n, r, H)
    x, gw = _rand(g, n, Cin), _rand(g, n, K * Cin)
    kp = _rand(g, K, 3) * 0.03
    kp[0] = 0
    extent = r * 1.2 / 2.5
    # the aggregation kernels: bit-equal valid rows, zero dead rows, NaN in every dead input row (x, q, s, dwf)
    xe = x.clone().requires_grad_(True)
    wf = ops._KPConvAgg.apply(xe, pts, pts, nbr, kp, extent, rev, off)
    w, cnt = wf.grad_fn.saved_tensors
    wf.backward(gw)
    xc = _pad(x).requires_grad_(True)
    pc = _pad(pts)
    wfc = ops._KPConvAgg.apply(xc, pc, pc, nbc, kp, extent, revc, off)
    wc, cntc = wfc.grad_fn.saved_tensors
    # rows 96..103 are one tile of the kernel: three live queries, five dead ones (the dead queries of a LIVE tile)
    assert n == 99 and torch.equal(wc[:n], w) and torch.equal(cntc[:n], cnt)
    assert bool((cntc[n:104] == 1).all()) and not bool(wc[n:104].any())
    assert bool((cntc[104:] == 1).all()) and not bool(wc[104:].any())       # the wholly dead tiles
    wfc.backward(_pad(gw))
    assert torch.equal(wfc[:n].detach(), wf.detach()) and not bool(wfc[n:].detach().any())
    assert torch.equal(xc.grad[:n], xe.grad) and not bool(xc.grad[n:].any())
    # the whole op (the library GEMM runs on all CAP rows): zero dead rows in, zero dead rows out, dW untouched by them.
    # Bound: the GEMM may sum its K*Cin <= 495 products in another order for 128 rows than for 99 -- 1e-5 of the largest
    # value is > 20x the worst fp32 reordering error of that many terms (495 * 2^-24 ~ 3e-5 relative to the SUM OF
    # MAGNITUDES is the hard bound; the values here are sums of signed terms of magnitude <= 1).
    W = _rand(g, K, Cin, Cout) * 0.2
    gy = _rand(g, n, Cout)
    We = W.clone().requires_grad_(True)
    xe = x.clone().requires_grad_(True)
    y = ops.kpconv(xe, pts, pts, nbr, rev, kp, We, extent, off)
    y.backward(gy)
    Wc = W.clone().requires_grad_(True)
    xc = _pad(x, fill=0.0).requires_grad_(True)             # invariant 1 holds for what the GEMM reads
    yc = ops.kpconv(xc, pc, pc, nbc, revc, kp, Wc, extent, off)
    yc.backward(_pad(gy, fill=0.0))
    assert not bool(yc[n:].detach().any()) and not bool(xc.grad[n:].any())
    for a, b in ((yc[:n].detach(), y.detach()), (xc.grad[:n], xe.grad), (Wc.grad, We.grad)):
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_seg_instnorm_cap_on_uneven_clouds(mode):
    from sug_amd import ops
    _, off, n, g = _case(mode)
    C = 70                                                  # two channel chunks, the second partial
    x, sc, gy = _rand(g, n, C) * 3 + 1, _rand(g, n, C), _rand(g, n, C)
    xe = x.clone().requires_grad_(True)
    se = sc.clone().requires_grad_(True) if mode == 2 else None
    y = ops.seg_instnorm(xe, off, act=mode == 1, shortcut=se)
    y.backward(gy)
    xc = _pad(x).requires_grad_(True)
    scc = _pad(sc).requires_grad_(True) if mode == 2 else None
    yc = ops.seg_instnorm(xc, off, act=mode == 1, shortcut=scc)
    yc.backward(_pad(gy))
    assert torch.equal(yc[:n].detach(), y.detach()) and not bool(yc[n:].detach().any())
    assert torch.equal(xc.grad[:n], xe.grad) and not bool(xc.grad[n:].any())
    if mode == 2:
        assert torch.equal(scc.grad[:n], se.grad) and not bool(scc.grad[n:].any())


def test_max_pool_mean_and_node_sampling_on_uneven_clouds():
    from sug_amd import ops
    from sug_amd.model.KPConv_blocks import sample_tensor_slices
    pts, off, n, g = _case(5)
    H, C = 10, 9
    nbr, rev, nbc, revc = _tables(pts, off, n, 0.08, H)
    x, gy = _rand(g, n, C) - 0.3, _rand(g, n, C)            # negatives: the zero shadow row can win
    xe = x.clone().requires_grad_(True)
    y = ops.seg_max_pool(xe, nbr, rev)
    y.backward(gy)
    xc = _pad(x).requires_grad_(True)
    yc = ops.seg_max_pool(xc, nbc, revc)                    # the one op serves both layouts (invariants 2 and 3)
    yc.backward(_pad(gy))
    assert torch.equal(yc[:n].detach(), y.detach()) and not bool(yc[n:].detach().any())
    assert torch.equal(xc.grad[:n], xe.grad) and not bool(xc.grad[n:].any())
    gm = _rand(g, len(LENS), C)
    xe = x.clone().requires_grad_(True)
    m = ops.seg_mean(xe, off)
    m.backward(gm)
    xc = _pad(x).requires_grad_(True)
    mc = ops.seg_mean(xc, off)
    mc.backward(gm)
    assert torch.equal(mc.detach(), m.detach())
    assert torch.equal(xc.grad[:n], xe.grad) and not bool(xc.grad[n:].any())
    assert torch.equal(ops.kp_sample_rows(_pad(x), off), sample_tensor_slices(x, LENS))


def test_empty_cloud_and_long_clouds():
    """Clouds [130, 0, 64] in 256 rows: the empty cloud normalises nothing, its mean row and node rows are zero; the other
    clouds equal the ops on the tight clouds [130, 64]; node sampling takes the stride rule for n >= 64."""
    from sug_amd import ops
    from sug_amd.model.KPConv_blocks import sample_tensor_slices
    g = torch.Generator().manual_seed(9)
    n, C = 194, 40
    off = torch.tensor([0, 130, 130, 194], dtype=torch.int32, device=DEV)
    off2 = torch.tensor([0, 130, 194], dtype=torch.int32, device=DEV)
    x, gy, gm = _rand(g, n, C), _rand(g, n, C), _rand(g, 3, C)
    xe = x.clone().requires_grad_(True)
    y = ops.seg_instnorm(xe, off2, act=True)
    y.backward(gy)
    xc = _pad(x, 256).requires_grad_(True)
    yc = ops.seg_instnorm(xc, off, act=True)
    yc.backward(_pad(gy, 256))
    assert torch.equal(yc[:n].detach(), y.detach()) and not bool(yc[n:].detach().any())
    assert torch.equal(xc.grad[:n], xe.grad) and not bool(xc.grad[n:].any())
    xe = x.clone().requires_grad_(True)
    m = ops.seg_mean(xe, off2)
    m.backward(gm[[0, 2]])
    xc = _pad(x, 256).requires_grad_(True)
    mc = ops.seg_mean(xc, off)
    mc.backward(gm)
    assert torch.equal(mc[[0, 2]].detach(), m.detach()) and not bool(mc[1].detach().any())
    assert torch.equal(xc.grad[:n], xe.grad) and not bool(xc.grad[n:].any())
    s = ops.kp_sample_rows(_pad(x, 256), off)
    assert torch.equal(s[[0, 2]], sample_tensor_slices(x, [130, 64])) and not bool(s[1].any())


def test_grid_subsample_tight_against_capacity_buffer():
    """One subsample, twice: into a buffer of as many rows as went in, without a record, and into one of CAP rows with a
    record.  The same offsets and valid rows, zero rows past the total in both, the total in the record."""
    from sug_amd import ops
    pts, off, n, _ = _case(2)
    B, dl = len(LENS), 0.08
    pt, ot = ops.kp_grid_subsample(pts, off, B, max(LENS), dl)
    rec = torch.zeros(ops.KPCONV_RECORD_INTS, dtype=torch.int32, device=DEV)
    pc, oc = ops.kp_grid_subsample(pts, off, B, max(LENS), dl, rows=CAP, record=rec, level=0)
    cnt = np.diff(ot.cpu().numpy())
    total = int(cnt.sum())
    assert all(0 < c < l for c, l in zip(cnt[[0, 2]], (LENS[0], LENS[2]))) and 0 < cnt[1] <= LENS[1] and total < n   # they shrink
    assert torch.equal(ot, oc)
    assert pt.shape == (n, 3) and pc.shape == (CAP, 3)
    assert torch.equal(pt[:total], pc[:total]) and bool(pt[:total].any())
    assert not bool(pt[total:].any()) and not bool(pc[total:].any())
    r = rec.tolist()
    assert r[0] == total and r[4] == 0


def test_reference_style_kpconv_call():
    """KPConv.forward(q, s, nbr, x) as the reference calls it -- no reverse lists, no offsets: one cloud's tables.  Value
    and input gradient equal ops.kpconv with the one-cloud offsets and lists spelled out."""
    from sug_amd import ops
    from sug_amd.model.KPConv_blocks import KPConv
    n, H, Cin, Cout, r = 60, 12, 16, 24, 0.08
    pts, off, _, g = _case(3, lens=[n])
    nbr = ops.radius_neighbors(pts, off, pts, off, r, H)
    torch.manual_seed(0)
    conv = KPConv(15, 3, Cin, Cout, r * 1.2 / 2.5, r).to(DEV)
    x, gy = _rand(g, n, Cin), _rand(g, n, Cout)
    xa = x.clone().requires_grad_(True)
    ya = conv(pts, pts, nbr.long(), xa)                     # (the reference's tables are int64)
    ya.backward(gy)
    xb = x.clone().requires_grad_(True)
    rev = ops.radius_reverse(nbr, off, off, n, n)
    yb = ops.kpconv(xb, pts, pts, nbr, rev, conv.kernel_points, conv.weights, conv.KP_extent, off)
    yb.backward(gy)
    assert bool(ya.detach().any()) and torch.equal(ya.detach(), yb.detach()) and torch.equal(xa.grad, xb.grad)


# ----------------------------------------------------------------------------------------------- 3. model parity
def _close(a, ref, tol=1e-4):
    ref = np.asarray(ref)
    err = np.abs(a.detach().cpu().numpy() - ref).max()
    assert err <= tol * max(1.0, np.abs(ref).max()), err


def test_models_with_caps_match_reference_in_every_mode():
    z = _gold()
    m = _model(caps=GOLD_CAPS)
    x = _x()
    with torch.no_grad():
        y1, y2 = m(x)
        _close(y1, z['y1'])
        _close(y2, z['y2'])
        for t, k in zip(m(x, semantic_adaption=True), ('sem_y1', 'sem_y2', 'sem_f1', 'sem_f2')):
            _close(t, z[k])
        _close(m(x, node_adaptation_s=True), z['node_s'])
        _close(m(x, node_adaptation_t=True), z['node_t'])
        gf, fo = m(x, mid_feat=True)
        _close(gf, z['mid_x'])
        _close(fo, z['mid_feat'])
        assert m(x, node_vis=True) is None
        y1a, _ = m(x, adaptation=True, constant=0.5)
        _close(y1a, z['y1'])
        _close(_model('cls', GOLD_CAPS)(x), z['cls_logits'])
    assert m.g.capacity_report()['overflows'] == 0


def _loss(m, x):
    sem = m(x, semantic_adaption=True)
    ns = m(x, node_adaptation_s=True)
    tot = 0
    for i, t in enumerate((sem[0], sem[1], sem[2], ns)):
        r = torch.randn(t.shape, generator=torch.Generator().manual_seed(100 + i), dtype=torch.float64).float()
        tot = tot + (t * r.to(DEV)).sum()
    return tot


def test_gradients_with_caps_as_accurate_as_reference_fp32():
    z = _gold()
    m = _model(caps=GOLD_CAPS)
    _loss(m, _x()).backward()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    names = list(z['grad_names'])
    assert sorted(grads) == names
    for k, n64, e32 in zip(names, z['grad_norm64'], z['grad_err32']):
        n = grads[k].double().norm().item()
        assert abs(n - n64) <= 4 * e32 + 1e-5 * n64 + 1e-12, (k, n, n64, e32)
    for key in z.files:
        if key.startswith('grad64:'):
            k = key[len('grad64:'):]
            g64, g32 = z[key], z['grad32:' + k]
            e_ours = np.linalg.norm(grads[k].cpu().double().numpy() - g64)
            e_ref = np.linalg.norm(g32.astype(np.float64) - g64)
            assert e_ours <= 4 * e_ref + 1e-6 * np.linalg.norm(g64) + 1e-12, (k, e_ours, e_ref)


# ----------------------------------------------------------------------------------------------- 4. no host wait
def test_preprocessing_forward_backward_in_one_graph():
    """A capture refuses every host wait: the whole of KPFCls with caps -- pyramid, forward, backward -- is captured on the
    first synthetic batch and replayed on the second, whose levels have other sizes; outputs and every gradient equal the
    eager run on that batch bit for bit."""
    from sug_amd import ops
    xs, caps, lengths = _synth()
    assert lengths[0][2] != lengths[1][2]                   # the batches differ in their level sizes
    m = _model('cls', caps)
    r = _rand(torch.Generator().manual_seed(4), 4, 10)
    params = [p for p in m.parameters() if p.requires_grad]

    def run(x):
        out = m(x)
        (out * r).sum().backward()
        return out

    def eager(x):
        for p in params:
            p.grad = None
        out = run(x).detach().clone()
        return out, [None if p.grad is None else p.grad.clone() for p in params]

    eager(xs[0])                                            # (the capacity record is made outside the capture)
    ref_out, ref_grads = eager(xs[1])
    for p in params:
        p.grad = None
    torch.cuda.synchronize()
    static = xs[0].clone()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard(), torch.cuda.graph(graph):
        out = run(static)
    static.copy_(xs[1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), ref_out)
    for p, gr in zip(params, ref_grads):
        assert (p.grad is None) == (gr is None)
        if gr is not None:
            assert torch.equal(p.grad, gr)
    assert m.capacity_report()['overflows'] == 0


# ----------------------------------------------------------------------------------------------- 5. the step objects
def _labels(B):
    return (torch.arange(B, device=DEV) % 10).long()


def _run_source(use_graph):
    from sug_amd.source_step import SourceStep
    xs, caps, _ = _synth()
    net = _model('cls', caps)
    tr = SourceStep(net, use_graph=use_graph)
    torch.manual_seed(11)
    rng = torch.get_rng_state()
    out = []
    for x in xs:
        out.append((float(tr.step(x, _labels(4))), _state_hash(net)))
    assert torch.equal(torch.get_rng_state(), rng)          # the KPConv step draws nothing from the CPU generator
    totals = tr.epoch_totals()                              # the epoch read: nothing overflowed
    return out, totals, tr


def test_source_step_replay_equals_eager():
    a, ta, _ = _run_source(False)
    b, tb, tr = _run_source(True)
    assert tr.why is None and tr.stats['captured'] == 1 and tr.stats['replayed'] == 2, (tr.why, tr.stats)
    assert a == b, (a, b)
    assert ta == tb and ta[1] == 12.0


def _run_sug(use_graph):
    from sug_amd.train_step import SUGStep
    xs, caps, _ = _synth()
    net = _model('net', caps)
    tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=use_graph, methods=bench.BENCH_METHODS)
    torch.manual_seed(3)
    rng = torch.get_rng_state()
    lab = _labels(2)
    out = []
    for x in xs:                                            # 2 clouds per domain: source = the first two, target = the others
        losses = [float(v) for v in tr.step(x[:2].contiguous(), lab, x[2:].contiguous(), lab)]
        out.append((losses, _state_hash(net)))
    assert torch.equal(torch.get_rng_state(), rng)
    rep = tr.epoch_check()
    assert rep['overflows'] == 0
    if use_graph:                                           # one key, captured: steps 2 and 3 were replays
        assert len(tr._graphs) == 1 and next(iter(tr._graphs.values()))['graph'] is not None
    return out


def test_sugstep_replay_equals_eager():
    a = _run_sug(False)
    c = _run_sug(True)
    assert a == c, 'graph replay differs from eager: %s vs %s' % ([x[0] for x in a], [x[0] for x in c])
    assert all(np.isfinite(v) for x in a for v in x[0])


def test_paired_form_leaves_the_generator_where_the_four_call_form_does():
    """forward_pair draws no FPS starts for an encoder that samples nothing: the CPU generator ends a SUG step where the
    four model(...) calls of an unchanged caller leave it -- untouched."""
    xs, caps, _ = _synth()
    net = _model('net', caps)
    x = xs[2]
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    with torch.no_grad():
        net(x[:2].contiguous(), semantic_adaption=True)
        net(x[2:].contiguous(), semantic_adaption=True)
        net(x[:2].contiguous(), node_adaptation_s=True)
        net(x[2:].contiguous(), node_adaptation_t=True)
        four = torch.get_rng_state()
        (s, t) = net.forward_pair(x)
        net.forward_pair(x, node_adaptation=True)
    assert torch.equal(four, rng) and torch.equal(torch.get_rng_state(), rng)
    # the paired form computes the four-call form's values for this encoder (its norm is per cloud).  Bound: the library
    # GEMMs run on twice the rows and may sum in another order -- fp32 rounding, 1e-5 of the largest value
    with torch.no_grad():
        ys = net(x[:2].contiguous(), semantic_adaption=True)
    for a, b in zip(s, ys):
        err = float((a - b).abs().max())
        print('paired vs four-call: max |diff| %.3e of max |value| %.3e' % (err, float(b.abs().max())))
        assert err <= 1e-5 * max(1.0, float(b.abs().max()))


def test_eval_graphs_replays_the_eval_forward_with_caps():
    from sug_amd import eval_graphs
    xs, caps, _ = _synth()
    m = _model('net', caps).eval()
    assert eval_graphs.fallback_reason(m, xs[0]) is None
    r = eval_graphs.runner_for(m)
    before = dict(r.stats)
    try:
        for x in (xs[0], xs[1], xs[2]):                     # eager (plan), capture + replay, replay
            got = eval_graphs.forward(m, x)
            with torch.no_grad():
                want = m(x)
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
        assert r.stats['replayed'] - before['replayed'] == 2 and r.stats['refused'] == before['refused'], (r.stats, r.why)
    finally:
        eval_graphs.drop_all()


def test_uda_step_and_call_graphs_decline_the_capacity_form():
    """Neither switches on as a side effect of graph_capturable: both decline the backbone with caps, with a reason."""
    from sug_amd import call_graphs
    from sug_amd.uda_step import UDAStep
    xs, caps, _ = _synth()
    net = _model('net', caps)
    assert net.g.graph_capturable is True and call_graphs.manager_for(net) is None
    tr = UDAStep(net, use_graph=True)
    assert not tr.use_graph and not tr.pair_domains and 'level caps are not supported by UDAStep' in tr.why


# ----------------------------------------------------------------------------------------------- 6. overflow (last)
def test_overflow_is_clamped_reported_and_leaves_no_trace():
    from sug_amd.model.KPConv_model import level_capacity
    from sug_amd.source_step import SourceStep
    xs, caps, lengths = _synth()
    need3 = sum(lengths[0][3])                              # level-3 rows of the scale-1.0 batch (about 4 * 205)
    assert need3 > level_capacity(4, 256, (caps[0], caps[1], 128, caps[3]))[3]
    # 6a. level 3 capped at 128 rows per cloud
    caps_a = (caps[0], caps[1], 128, caps[3])
    m = _model('cls', caps_a)
    out = m(xs[0])
    out.sum().backward()
    assert bool(torch.isfinite(out).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    rep = m.capacity_report()
    assert rep['overflows'] == 1
    lv = rep['levels'][2]
    assert lv['level'] == 3 and lv['needed'] == need3 > lv['capacity'] == 512
    assert level_capacity(4, 256, (caps[0], caps[1], lv['cap_needed'], caps[3]))[3] >= need3      # the named cap suffices
    assert all(r['needed'] <= r['capacity'] for r in rep['levels'][:2])
    tr = SourceStep(_model('cls', caps_a), use_graph=False)
    tr.step(xs[0], _labels(4))
    with pytest.raises(RuntimeError, match=r'level 3 needed %d rows' % need3):
        tr.epoch_totals()
    tr.epoch_totals()                                       # the read cleared the record
    # 6b. level 4 holds 64 rows in all: the last cloud is dropped whole
    assert sum(lengths[0][4][:3]) >= 64
    net = _model('net', (caps[0], caps[1], caps[2], 1))
    feats, nodes = net.g(xs[0])
    feats.sum().backward()
    assert bool(torch.isfinite(feats).all()) and bool(torch.isfinite(nodes).all())
    assert not bool(feats[-1].any())                        # an empty cloud's pooled row is zero
    assert bool(feats[0].any())
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.g.parameters() if p.grad is not None)
    rep = net.g.capacity_report()
    assert rep['overflows'] == 1 and rep['levels'][3]['needed'] == sum(lengths[0][4]) > rep['levels'][3]['capacity'] == 64
    # 6c. afterwards a batch that fits gives what a fresh model gives
    m.set_level_caps(caps)
    for p in m.parameters():
        p.grad = None
    fresh = _model('cls', caps)
    for x in (xs[0], xs[1]):
        assert torch.equal(m(x), fresh(x))
    assert m.capacity_report()['overflows'] == 0
