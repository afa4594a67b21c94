"""GPU: sug_pfh_descriptors, sug_pfh_hist_distance, sug_amd.utils.pfh and split_dataset_geometric(metric='pfh') against
the reference's results in tests/golden/pfh.npz and, where the reference cannot run, against the numpy restatement
tests/pfh_cases.py.

Bounds (tests/test_pfh_host.py derives them): counts and neighbour lists EXACT -- the fixture keeps every discrete decision
1e-9 from flipping --, normals within 64 * 2^-52 / gap per point, distances within (D + 2) * 2^-52 relative.  The
restatement-only clouds contain rank-deficient neighbourhoods, whose normals nothing pins: there the kernel's histogram is
held against the restatement's binning of the KERNEL's own normals, on clouds whose margins the test asserts."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import pfh_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(GOLDEN, 'pfh.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _describe(dev, pts, rad, k, div):
    from sug_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(dev)
    out = ops.pfh_descriptors(x if x.dim() == 3 else x.unsqueeze(0), rad, k, div)
    return dict(zip(('hist', 'normals', 'idx', 'cnt', 'used'), (o.cpu().numpy() for o in out)))


@pytest.fixture(scope='module')
def runs(fx, dev):
    """Every golden case launched once, alone: {name: {output: numpy array without the batch axis}}."""
    out = {}
    for name, (N, rad, div, k) in C.CASES.items():
        out[name] = {key: v[0] for key, v in _describe(dev, fx[name + '_pts'], rad, k, div).items()}
    return out


@pytest.mark.parametrize('name', list(C.CASES))
def test_golden_descriptors(fx, runs, name):
    N, rad, div, k = C.CASES[name]
    got = runs[name]
    assert got['hist'].dtype == np.float64 and got['hist'].shape == (N, div ** 3) and got['idx'].dtype == np.int32
    assert got['used'] == N
    assert np.array_equal(got['idx'], fx[name + '_nbr'])
    assert np.array_equal(got['cnt'], (fx[name + '_nbr'] >= 0).sum(axis=1))
    assert np.array_equal(got['hist'], fx[name + '_counts'] / float(C.npairs(k)))          # bit for bit numpy's division
    err = np.abs(got['normals'] - fx[name + '_normals']).max(axis=1)
    bound = C.normal_bound(fx[name + '_gap'])
    print('%s: largest normal error %.2e, in units of its bound %.3f' % (name, err.max(), (err / bound).max()))
    assert (err <= bound).all()


def test_golden_distances(fx, runs, dev):
    from sug_amd import ops
    from sug_amd.utils import pfh
    t = {name: (torch.from_numpy(r['hist']).to(dev), torch.from_numpy(r['cnt']).to(dev)) for name, r in runs.items()}
    keys = [k for k in fx if k.startswith('dist_')]
    assert len(keys) == 18
    for key in keys:
        s, d = key[len('dist_'):].split('__')                                              # Ns != Nt in most of them
        got = ops.pfh_hist_distance(t[s][0], t[s][1], t[d][0].unsqueeze(0), t[d][1].unsqueeze(0))
        ref = float(fx[key])
        print('%s: %.17g, relative error %.2e' % (key, got.item(), abs(got.item() - ref) / ref if ref else 0.0))
        assert got.shape == (1,) and abs(got.item() - ref) <= C.distance_bound(C.CASES[s][2] ** 3) * ref
        if s == d:
            assert got.item() == 0.0                                                       # self-distance exactly 0
        assert pfh.pfh_hist_distance(t[s][0], t[d][0]).item() == got.item()                # utils: used rows from the rows


@pytest.mark.parametrize('name', list(C.CASES))
def test_golden_through_utils(fx, runs, dev, name):
    from sug_amd.utils import pfh
    N, rad, div, k = C.CASES[name]
    pc = torch.from_numpy(fx[name + '_pts']).to(dev)
    d = pfh.PFH(0.1, div, k, rad)
    normals, lists, used = d.calc_normals(pc)
    hist = d.calcHistArray(pc, normals, lists, used)
    assert used.dtype == torch.bool and bool(used.all()) and hist.shape == (N, div ** 3)
    assert np.array_equal(hist.cpu().numpy(), runs[name]['hist']) and np.array_equal(lists.cpu().numpy(), runs[name]['idx'])
    assert np.array_equal(normals.cpu().numpy(), runs[name]['normals'])
    assert torch.equal(d.calcHistArray(pc), hist) and torch.equal(pfh.PFH(0.1, div, k, rad).calcHistArray(pc), hist)
    with pytest.raises(ValueError, match='calc_normals'):
        d.calcHistArray(pc, normals.clone(), lists, used)
    batched = d.calc_normals(pc.unsqueeze(0).expand(2, -1, -1))
    assert batched[0].shape == (2, N, 3) and torch.equal(batched[0][1], normals) and torch.equal(batched[2][0], used)


def test_get_pfh_descriptor_is_one_launch_of_the_reference_parameters(fx, runs, dev):
    from sug_amd import ops
    from sug_amd.utils import pfh
    pcs = torch.from_numpy(np.stack((fx['c500_d2_pts'], fx['c500_d2_pts'][::-1].copy()))).to(dev)
    with ops.CTX.scoped(profile={}) as ctx:
        hists, status = pfh.get_pfh_descriptor(pcs, 'modelnet')
        launches = {name: len(events) for name, events in ctx.profile.items()}
    assert launches == {'pfh_descriptors': 1}
    assert status.tolist() == [True, True] and hists.shape == (2, 500, 8)
    assert np.array_equal(hists[0].cpu().numpy(), runs['c500_d2']['hist'])                 # (0.1, 2, 8, 0.2)
    # the reversed cloud: the same histograms, rows reversed (every margin of the fixture holds under a permutation)
    assert np.array_equal(hists[1].cpu().numpy()[::-1], runs['c500_d2']['hist'])


def test_batch_independent_and_deterministic(fx, runs, dev):
    """M = 3, a different cloud per block: each cloud's outputs bitwise equal to its M = 1 launch and to a second run."""
    pts = np.stack((fx['c64_d2_pts'], fx['c64_d3_pts'], fx['c64_d2_pts'][::-1]))
    N, rad, div, k = C.CASES['c64_d2']
    first, second = _describe(dev, pts, rad, k, div), _describe(dev, pts, rad, k, div)
    for key in first:
        assert np.array_equal(first[key], second[key]), key
    alone = [_describe(dev, pts[m], rad, k, div) for m in range(3)]
    for m in range(3):
        for key in first:
            assert np.array_equal(first[key][m], alone[m][key][0]), (m, key)
    for key in ('hist', 'normals', 'idx', 'cnt'):
        assert np.array_equal(first[key][0], runs['c64_d2'][key]), key
    assert not np.array_equal(first['hist'][0], first['hist'][1])
    # 500 points: two points per lane
    big = np.stack((fx['c500_d2_pts'], fx['c500_d2_pts'][::-1]))
    both = _describe(dev, big, 0.2, 8, 2)
    assert np.array_equal(both['hist'][0], runs['c500_d2']['hist']) and np.array_equal(both['normals'][0], runs['c500_d2']['normals'])
    assert np.array_equal(both['hist'][1], runs['c500_d2']['hist'][::-1])


# ------------------------------------------------------------------------------------- where the reference cannot run
def _cloud(kind):
    g = np.random.default_rng({'isolated': 1, 'five': 2, 'duplicate': 3, 'wide': 4, 'k16': 5, 'lone': 6, 'big': 7}[kind])
    if kind == 'isolated':                   # point 17 far from the shell: unused
        P = C.shell(70, g)
        P[17] = (3.0, 3.0, 3.0)
        return P, 0.45, 8, 2
    if kind == 'five':                       # N = 5 < k + 1
        return C.shell(5, g), 4.0, 8, 3
    if kind == 'duplicate':                  # points 40 and 9 coincide: 40 is its own neighbour, NaN features
        P = C.shell(64, g)
        P[40] = P[9]
        return P, 0.45, 8, 2
    if kind == 'wide':                       # rad = 0.9 on a sparse cloud: |a|, |b| > 1 occur, the arccos comparison is false
        return C.shell(14, g), 0.9, 8, 2
    if kind == 'k16':
        return C.shell(150, g), 0.5, 16, 4
    if kind == 'big':                        # 1024 points, 16 neighbours, div 5: the largest LDS footprint, four points per lane
        return C.shell(1024, g), 0.2, 16, 5
    return (g.uniform(-1, 1, (12, 3)) * 40).astype(np.float32), 0.2, 8, 2                  # 'lone': no point has a neighbour


@pytest.mark.parametrize('kind', ['isolated', 'five', 'duplicate', 'wide', 'k16', 'lone', 'big'])
def test_restatement_only_cases(dev, kind):
    P, rad, k, div = _cloud(kind)
    P64 = P.astype(np.float64)
    got = {key: v[0] for key, v in _describe(dev, P, rad, k, div).items()}
    idx, cnt, m_n = C.neighbours(P64, rad, k)
    assert m_n >= C.MARGIN or kind == 'duplicate'          # the duplicate's tie is decided by the index, not by rounding
    assert np.array_equal(got['idx'], idx) and np.array_equal(got['cnt'], cnt) and got['used'] == (cnt > 0).sum()
    unused = cnt == 0
    assert not got['hist'][unused].any() and not got['normals'][unused].any()
    assert np.isfinite(got['normals']).all()
    np.testing.assert_allclose(np.linalg.norm(got['normals'][~unused], axis=1), 1.0, rtol=0, atol=1e-14)
    P_dot = (got['normals'] * P64).sum(axis=1)
    assert (P_dot <= 1e-15).all()                                                          # oriented: normal . (-p) >= 0
    # the histogram: the restatement's binning of the kernel's normals
    counts, m_h, ab_max = C.hist_counts(P64, got['normals'], idx, cnt, div)
    assert m_h >= C.MARGIN, m_h
    assert np.array_equal(got['hist'], counts / float(C.npairs(k)))
    # the normals where they are pinned: three or more neighbours and an eigen gap
    nrm, gap, dots = C.normals(P64, idx, cnt)
    pinned = (cnt >= 3) & (gap >= C.GAP) & (dots >= C.MARGIN)
    err = np.abs(got['normals'] - nrm).max(axis=1)
    if pinned.any():
        print('%s: %d used, %d pinned normals, largest error in units of the bound %.3f'
              % (kind, (~unused).sum(), pinned.sum(), (err[pinned] / C.normal_bound(gap[pinned])).max()))
        assert (err[pinned] <= C.normal_bound(gap[pinned])).all()
    last = div ** 3 - 1
    if kind == 'isolated':
        assert cnt[17] == 0 and (cnt > 0).sum() == 69 and not (idx == 17).any()
    elif kind == 'five':
        assert (cnt == 4).all() and np.allclose(got['hist'].sum(axis=1), 10 / 36.0)        # comb(5, 2) pairs of comb(9, 2)
    elif kind == 'duplicate':
        assert idx[40, 0] == 40 and idx[9, 0] == 40 and got['hist'][40, last] > 0          # the NaN pair in the last bin
    elif kind == 'wide':
        assert ab_max > 1 + C.MARGIN                                                       # the route is taken
    elif kind == 'k16':
        assert cnt.max() == 16 and np.allclose(got['hist'][cnt == 16].sum(axis=1), 1.0)
    elif kind == 'big':
        assert cnt.max() == 16 and got['used'] == 1024
    else:
        assert got['used'] == 0 and not got['hist'].any() and (idx == -1).all()


def test_distance_variants(fx, runs, dev):
    from sug_amd import ops
    P, rad, k, div = _cloud('isolated')
    iso = {key: v[0] for key, v in _describe(dev, P, rad, k, div).items()}                 # 69 used rows: odd
    lone = {key: v[0] for key, v in _describe(dev, *_cloud('lone')).items()}
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sets = {'iso': iso, 'c64': runs['c64_d2'], 'c130': runs['c130_d2']}                    # used counts 69, 64, 130
    for s in sets:
        for t in sets:
            got = ops.pfh_hist_distance(to(sets[s]['hist']), to(sets[s]['cnt']), to(sets[t]['hist'][None]), to(sets[t]['cnt'][None])).item()
            ref = C.hist_distance(sets[s]['hist'], sets[s]['cnt'] > 0, sets[t]['hist'], sets[t]['cnt'] > 0)
            assert abs(got - ref) <= C.distance_bound(8) * ref, (s, t)
            assert (got == 0.0) == (s == t)
    # the unused row takes no part: dropping it from the arrays changes nothing
    keep = iso['cnt'] > 0
    a = ops.pfh_hist_distance(to(iso['hist']), to(iso['cnt']), to(runs['c64_d2']['hist'][None]), to(runs['c64_d2']['cnt'][None]))
    b = ops.pfh_hist_distance(to(iso['hist'][keep]), to(iso['cnt'][keep]), to(runs['c64_d2']['hist'][None]), to(runs['c64_d2']['cnt'][None]))
    assert a.item() == b.item()
    a = ops.pfh_hist_distance(to(runs['c64_d2']['hist']), to(runs['c64_d2']['cnt']), to(iso['hist'][None]), to(iso['cnt'][None]))
    b = ops.pfh_hist_distance(to(runs['c64_d2']['hist']), to(runs['c64_d2']['cnt']), to(iso['hist'][keep][None]), to(iso['cnt'][keep][None]))
    assert a.item() == b.item()
    # no used row on either side: NaN
    src, tgt = (to(runs['c64_d2']['hist']), to(runs['c64_d2']['cnt'])), (to(lone['hist'][None]), to(lone['cnt'][None]))
    assert np.isnan(ops.pfh_hist_distance(src[0], src[1], tgt[0], tgt[1]).item())
    assert np.isnan(ops.pfh_hist_distance(tgt[0][0], tgt[1][0], src[0][None], src[1][None]).item())
    # one source against B targets: stride 0 == the repeated source, bit for bit, and == pair by pair
    ht = to(np.stack((runs['c64_d2']['hist'], runs['c64_d3']['hist'][:, :8], iso['hist'][:64])))
    ct = to(np.stack((runs['c64_d2']['cnt'], runs['c64_d3']['cnt'], iso['cnt'][:64])))
    one = ops.pfh_hist_distance(src[0], src[1], ht, ct)
    rep = ops.pfh_hist_distance(src[0][None].expand(3, -1, -1), src[1][None].expand(3, -1), ht, ct)
    assert one.shape == (3,) and torch.equal(one, rep) and one[0].item() == 0.0
    for m in range(3):
        assert ops.pfh_hist_distance(src[0], src[1], ht[m:m + 1], ct[m:m + 1]).item() == one[m].item()
    # D = 27, 64, 125: the row-in-registers and the re-read variants against the restatement
    g = np.random.default_rng(11)
    for D in (27, 64, 125):
        hs, hT = g.integers(0, 5, (33, D)) / 36.0, g.integers(0, 5, (2, 70, D)) / 36.0
        cs, cT = (g.uniform(size=33) < 0.8).astype(np.int32), (g.uniform(size=(2, 70)) < 0.8).astype(np.int32)
        got = ops.pfh_hist_distance(to(hs), to(cs), to(hT), to(cT)).cpu().numpy()
        for m in range(2):
            ref = C.hist_distance(hs, cs > 0, hT[m], cT[m] > 0)
            assert abs(got[m] - ref) <= C.distance_bound(D) * ref, (D, m)


def _flat_shell(P, g):
    """A shell squeezed to a needle: after process_pts 64 of its points lie closer than the reference's rad = 0.2."""
    v = g.standard_normal((P, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    axes = np.array([1.0, g.uniform(0.08, 0.3), g.uniform(0.04, 0.15)])
    return (v * g.uniform(0.7, 1.0, (P, 1)) * axes * g.uniform(0.5, 2.0) + g.uniform(-1, 1, 3)).astype(np.float32)


def test_split_dataset_geometric_pfh(dev):
    """2 classes x 8 shell clouds, pt_num = 64, given anchors.  The needles' tips have one or two neighbours, whose normals
    nothing pins, so the chain is checked link by link: the lists against the restatement, the histograms against the
    restatement's binning of the kernel's normals, and the split against _split_class fed by the restatement's distances
    between those histograms.  One cloud has an isolated point."""
    from sug_amd import dataset_splitter as S, ops
    g = np.random.default_rng(23)
    raw = np.stack([_flat_shell(96, g) for _ in range(16)])
    labels = np.array([0, 1] * 8)
    anchors = [[2, 3, 1, 0, 2], [3, 2, 1, 0, 3]]
    pts = torch.from_numpy(raw).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        split = S.split_dataset_geometric(pts, labels, num_class=2, anchors=anchors, pt_num=64, metric='pfh')
        icp = S.split_dataset_geometric(pts, labels, num_class=2, anchors=anchors, pt_num=64, metric='icp')
        plain = S.split_dataset_geometric(pts, labels, num_class=2, anchors=anchors, pt_num=64)
    for a, b in zip(icp, plain):                                                           # the default is untouched
        for x, y in zip(a, b):
            assert torch.equal(x, y) if torch.is_tensor(x) else x == y
    used_counts = []
    for cls in (0, 1):
        order = split.indices[cls]
        assert torch.equal(order, icp.indices[cls])
        processed = S.process_pts(pts.index_select(0, order), 64)
        hist, normals, idx, cnt, used = (o.cpu().numpy() for o in ops.pfh_descriptors(processed, S.PFH_RAD, S.PFH_NNEIGHBORS, S.PFH_DIV))
        used_counts += used.tolist()
        for m, cloud in enumerate(processed.cpu().numpy().astype(np.float64)):
            r_idx, r_cnt, m_n = C.neighbours(cloud, S.PFH_RAD, S.PFH_NNEIGHBORS)
            counts, m_h, _ = C.hist_counts(cloud, normals[m], r_idx, r_cnt, S.PFH_DIV)
            assert m_n >= C.MARGIN and m_h >= C.MARGIN, (cls, m, m_n, m_h)
            assert np.array_equal(idx[m], r_idx) and np.array_equal(hist[m], counts / 36.0), (cls, m)

        def distance_of(a):
            return np.array([C.hist_distance(hist[a], cnt[a] > 0, hist[m], cnt[m] > 0) for m in range(8)])
        given = iter(anchors[cls])
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            labels_c, d, anchor, tries = S._split_class(8, distance_of, lambda: next(given))
        got = split.distances[cls].cpu().numpy()
        print('class %d: tries %d, anchor %d, distances %s' % (cls, tries, anchor, got.tolist()))
        assert (np.abs(got - d) <= C.distance_bound(8) * d).all() and got[anchor] == 0.0
        assert (split.tries[cls], split.anchors[cls]) == (tries, anchor)
        assert np.array_equal(split.cluster_labels[cls].cpu().numpy(), S._geometric_labels(got)[0])
        assert np.array_equal(split.cluster_labels[cls].cpu().numpy(), labels_c)
        assert 0 < (labels_c == 0).sum() < 8
    assert min(used_counts) < 64 <= max(used_counts)                                       # an unused point took no part
