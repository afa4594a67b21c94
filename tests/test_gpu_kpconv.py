"""GPU: the KPConv backbone (sug_amd/csrc/kpconv.hip) -- preprocessing against the reference's pyramid, the kernels
against fp64 restatements, Net_MDA('KPConv') / KPFCls against the reference's outputs and gradients
(tests/golden/kpconv.npz, tests/golden/make_kpconv_goldens.py), run-to-run determinism and the unchanged caller."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, 'tests', 'golden', 'kpconv.npz')
DEV = 'cuda'


def _gold():
    return np.load(GOLD)


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int64)).tobytes()).hexdigest()


def _model(tag='net'):
    from oracle.ref_cpu import fill_params
    from sug_amd.model.Model import Net_MDA
    from sug_amd.model.KPConv_model import KPFCls
    z = _gold()
    shapes = {k: tuple(int(s) for s in sh.split(',') if s) for k, sh in zip(z[tag + '_keys'], z[tag + '_shapes'])}
    sd = fill_params(shapes, 7)
    for k, v in zip(z[tag + '_kp_keys'], z[tag + '_kp']):
        sd[k] = torch.from_numpy(v)
    m = Net_MDA('KPConv') if tag == 'net' else KPFCls()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train()


def _x():
    return torch.from_numpy(_gold()['x']).to(DEV)


# ----------------------------------------------------------------------------------------------- preprocessing
def _cpu_subsample(p, dl):
    """CPU restatement of the grid subsample of one cloud (first-occurrence order, fp32 point-order mean)."""
    keys = np.floor(p / np.float32(dl)).astype(np.int64)
    acc, order = {}, []
    for j, k in enumerate(map(tuple, keys)):
        if k not in acc:
            acc[k] = [np.float32(0)] * 3 + [0]
            order.append(k)
        a = acc[k]
        for ax in range(3):
            a[ax] = np.float32(a[ax] + p[j, ax])
        a[3] += 1
    return np.array([[acc[k][ax] / np.float32(acc[k][3]) for ax in range(3)] for k in order], dtype=np.float32)


def test_preprocessing_matches_reference_pyramid():
    from sug_amd.model.KPConv_model import PreprocessorGPU, KPConvConfig
    z = _gold()
    x = _x()
    B, N = x.shape[0], x.shape[2]
    pts = x.squeeze(-1).permute(0, 2, 1).reshape(B * N, 3).contiguous()
    meta = PreprocessorGPU(KPConvConfig).forward_packed(pts, [N] * B)
    L = int(z['levels'])
    assert len(meta['points']) == L
    for l in range(L):
        assert np.array_equal(meta['stack_lengths'][l].cpu().numpy(), z['lengths_%d' % l]), l
        assert np.array_equal(meta['points'][l].cpu().numpy(), z['points_%d' % l]), l        # bit-exact
        assert _sha(meta['neighbors'][l]) == str(z['neighbors_sha_%d' % l]), l
        if l < L - 1:
            assert _sha(meta['pools'][l]) == str(z['pools_sha_%d' % l]), l
            assert _sha(meta['upsamples'][l]) == str(z['upsamples_sha_%d' % l]), l
    # the CPU restatement of the subsample, cloud by cloud, on level 0 -> 1
    p0 = z['points_0'].reshape(B, N, 3)
    sub = np.concatenate([_cpu_subsample(p0[b], 2 * 0.05 / 2.5) for b in range(B)])
    assert np.array_equal(sub, z['points_1'])


# ----------------------------------------------------------------------------------------------- kernels vs fp64
def _case(seed=0):
    """Uneven clouds (incl. a 2-point cloud), shadow slots, a query without neighbours, negative features."""
    g = torch.Generator().manual_seed(seed)
    lens = [37, 2, 60]
    pts = torch.rand(sum(lens), 3, generator=g) * 0.2
    pts[lens[0] - 1] += 5.0                                  # isolated point: only itself within the radius
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return pts, off, lens


def _ref_nbr(pts, off, r, H):
    Ns = pts.shape[0]
    out = torch.full((Ns, H), Ns, dtype=torch.int64)
    for b in range(len(off) - 1):
        s0, s1 = int(off[b]), int(off[b + 1])
        for i in range(s0, s1):
            m = 0
            for j in range(s0, s1):
                d = pts[j] - pts[i]
                if ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < np.float32(r) * np.float32(r) and m < H:
                    out[i, m] = j
                    m += 1
    return out


@pytest.mark.parametrize('Cin', [1, 16, 33])
def test_kpconv_op_against_fp64(Cin):
    from sug_amd import ops
    pts, off, lens = _case(Cin)
    H, K, Cout, r = 12, 15, 24, 0.08
    nbr = _ref_nbr(pts, off, r, H)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(pts.shape[0], Cin, generator=g)                       # negative rows exercise the count quirk
    kp = torch.randn(K, 3, generator=g) * 0.03
    kp[0] = 0
    W = torch.randn(K, Cin, Cout, generator=g) * 0.2
    gy = torch.randn(pts.shape[0], Cout, generator=g)
    extent = r * 1.2 / 2.5
    # fp64 restatement (model/KPConv_blocks.py:302-447, rigid / linear / sum)
    xd, Wd = x.double().requires_grad_(True), W.double().requires_grad_(True)
    sp = torch.cat((pts.double(), torch.full((1, 3), 1e6, dtype=torch.float64)))
    xs = torch.cat((xd, torch.zeros(1, Cin, dtype=torch.float64)))
    nb = sp[nbr] - pts.double().unsqueeze(1)
    dist = (nb.unsqueeze(2) - kp.double()).pow(2).sum(3).sqrt()
    w = torch.clamp(1 - dist / extent, min=0).transpose(1, 2)
    nx = xs[nbr]
    outd = (torch.matmul(w, nx).permute(1, 0, 2) @ Wd).sum(0)
    cnt = torch.clamp((nx.sum(-1) > 0).sum(-1), min=1)
    outd = outd / cnt.unsqueeze(1)
    outd.backward(gy.double())
    # the build
    q = pts.to(DEV)
    o = off.to(DEV)
    n32 = nbr.to(torch.int32).to(DEV)
    rev = ops.radius_reverse(n32, o, o, pts.shape[0], max(lens))
    xg, Wg = x.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
    y = ops.kpconv(xg, q, q, n32, rev, kp.to(DEV), Wg, extent, o)
    y.backward(gy.to(DEV))
    scale = outd.abs().max().item()
    assert (y.detach().cpu().double() - outd.detach()).abs().max().item() <= 2e-6 * max(1.0, scale)
    assert (xg.grad.cpu().double() - xd.grad).abs().max().item() <= 2e-5 * max(1.0, xd.grad.abs().max().item())
    assert (Wg.grad.cpu().double() - Wd.grad).abs().max().item() <= 2e-5 * max(1.0, Wd.grad.abs().max().item())
    # the radius query on the same case
    assert torch.equal(ops.radius_neighbors(q, o, q, o, r, H).cpu().long(), nbr)


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_seg_instnorm_against_fp64(mode):
    from sug_amd import ops
    lens = [2, 50, 7, 131]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    g = torch.Generator().manual_seed(mode)
    C = 70
    x = torch.randn(sum(lens), C, generator=g) * 3 + 1
    sc = torch.randn(sum(lens), C, generator=g)
    gy = torch.randn(sum(lens), C, generator=g)
    def ref(dtype):
        xd, scd = x.to(dtype).clone().requires_grad_(True), sc.to(dtype).clone().requires_grad_(True)
        parts = []
        for b in range(len(lens)):
            s = xd[int(off[b]):int(off[b + 1])]
            parts.append((s - s.mean(0)) / torch.sqrt(s.var(0, unbiased=False) + 1e-5))
        yd = torch.cat(parts)
        if mode == 2:
            yd = yd + scd
        if mode >= 1:
            yd = torch.nn.functional.leaky_relu(yd, 0.1)
        yd.backward(gy.to(dtype))
        return yd.detach().double(), xd.grad.double(), scd.grad
    yd, dxd, dscd = ref(torch.float64)
    _, dx32, _ = ref(torch.float32)
    xg = x.to(DEV).requires_grad_(True)
    scg = sc.to(DEV).requires_grad_(True) if mode == 2 else None
    y = ops.seg_instnorm(xg, off.to(DEV), act=mode == 1, shortcut=scg)
    y.backward(gy.to(DEV))
    assert (y.detach().cpu().double() - yd).abs().max().item() < 1e-5
    # a 2-row segment's norm is ill-conditioned: as accurate as torch's own fp32 path, per segment
    for b in range(len(lens)):
        sl = slice(int(off[b]), int(off[b + 1]))
        e_ours = (xg.grad.cpu().double()[sl] - dxd[sl]).abs().max().item()
        e_t32 = (dx32[sl] - dxd[sl]).abs().max().item()
        assert e_ours <= 4 * e_t32 + 1e-5 * max(1.0, dxd[sl].abs().max().item()), (b, e_ours, e_t32)
    if mode == 2:
        assert (scg.grad.cpu().double() - dscd).abs().max().item() < 1e-6


def test_seg_max_pool_and_mean_against_fp64():
    from sug_amd import ops
    pts, off, lens = _case(5)
    H, C = 10, 9
    nbr = _ref_nbr(pts, off, 0.08, H)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(pts.shape[0], C, generator=g) - 0.3                  # negatives: the zero shadow row can win
    gy = torch.randn(pts.shape[0], C, generator=g)
    xd = x.double().requires_grad_(True)
    yd = torch.cat((xd, torch.zeros(1, C, dtype=torch.float64)))[nbr].max(1)[0]
    yd.backward(gy.double())
    n32 = nbr.to(torch.int32).to(DEV)
    o = off.to(DEV)
    rev = ops.radius_reverse(n32, o, o, pts.shape[0], max(lens))
    xg = x.to(DEV).requires_grad_(True)
    y = ops.seg_max_pool(xg, n32, rev)
    y.backward(gy.to(DEV))
    assert torch.equal(y.detach().cpu(), yd.detach().float())
    assert (xg.grad.cpu().double() - xd.grad).abs().max().item() < 1e-6
    xg2 = x.to(DEV).requires_grad_(True)
    m = ops.seg_mean(xg2, o)
    gm = torch.randn(m.shape, generator=g)
    m.backward(gm.to(DEV))
    md = torch.stack([x[int(off[b]):int(off[b + 1])].double().mean(0) for b in range(len(lens))])
    assert (m.detach().cpu().double() - md).abs().max().item() < 1e-6
    dd = torch.cat([gm[b].double().expand(lens[b], C) / lens[b] for b in range(len(lens))])
    assert (xg2.grad.cpu().double() - dd).abs().max().item() < 1e-6


# ----------------------------------------------------------------------------------------------- full model
def _close(a, ref, tol=1e-4):
    ref = np.asarray(ref)
    err = np.abs(a.detach().cpu().numpy() - ref).max()
    assert err <= tol * max(1.0, np.abs(ref).max()), err


def test_net_mda_kpconv_all_modes_match_reference():
    z = _gold()
    m = _model()
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
        _close(_model('cls')(x), z['cls_logits'])


def _loss(m, x):
    sem = m(x, semantic_adaption=True)
    ns = m(x, node_adaptation_s=True)
    tot = 0
    for i, t in enumerate((sem[0], sem[1], sem[2], ns)):
        r = torch.randn(t.shape, generator=torch.Generator().manual_seed(100 + i), dtype=torch.float64).float()
        tot = tot + (t * r.to(DEV)).sum()
    return tot


def test_net_mda_kpconv_gradients_as_accurate_as_reference_fp32():
    z = _gold()
    m = _model()
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


def test_kpconv_run_to_run_bit_identical():
    outs, hs = [], []
    for _ in range(2):
        m = _model()
        x = _x()
        y = m(x, semantic_adaption=True)
        _loss(m, x).backward()
        outs.append(torch.cat([t.detach().reshape(-1) for t in y]).cpu())
        h = hashlib.sha256()
        for k, p in m.named_parameters():
            if p.grad is not None:
                h.update(p.grad.detach().cpu().numpy().tobytes())
        hs.append(h.hexdigest())
    assert torch.equal(outs[0], outs[1])
    assert hs[0] == hs[1]


def _two_steps(call_graphs):
    from sug_amd.model.Model import Net_MDA
    m = _model()
    keep = Net_MDA.call_graphs
    Net_MDA.call_graphs = call_graphs
    try:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        x = _x()
        xs, xt = x, x.flip(2).contiguous()
        label = torch.arange(x.shape[0], device=DEV) % 10
        ce = torch.nn.CrossEntropyLoss()
        losses = []
        for _ in range(2):
            opt.zero_grad()
            y1, y2, f1, f2 = m(xs, semantic_adaption=True)
            t1, t2, g1, g2 = m(xt, semantic_adaption=True)
            ns = m(xs, node_adaptation_s=True)
            nt = m(xt, node_adaptation_t=True)
            loss = ce(y1, label) + ce(y2, label) + (f1 - g1).pow(2).mean() + (ns - nt).pow(2).mean()
            loss.backward()
            opt.step()
            losses.append(loss.detach().cpu())
        return torch.stack(losses), [p.detach().cpu().clone() for p in m.parameters()]
    finally:
        Net_MDA.call_graphs = keep


def test_unchanged_caller_call_graphs_auto_is_eager():
    from sug_amd import call_graphs
    from sug_amd.model.Model import Net_MDA
    assert call_graphs.manager_for(Net_MDA('KPConv').to(DEV)) is None
    la, pa = _two_steps('auto')
    lb, pb = _two_steps(False)
    assert torch.equal(la, lb)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_eval_takes_the_eager_form():
    from sug_amd import eval_graphs
    m = _model().eval()
    assert 'KPConv' in eval_graphs.fallback_reason(m, _x())
    with torch.no_grad():
        a = m(_x())[0]
        b = m(_x())[0]
    assert torch.equal(a, b)
