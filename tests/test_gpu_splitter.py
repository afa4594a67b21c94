"""GPU: sug_icp_fitness and sug_amd.dataset_splitter against the numpy fp64 restatement recorded in
tests/golden/splitter.npz (tests/splitter_cases.py, tests/golden/make_splitter_goldens.py).

The bounds: counts are integers and the fixture keeps every nearest-neighbour d2 at least 1e-9 relative away from r*r, so
an evaluation of the SAME points gives EQUAL counts; an fp64 sum of at most 1024 positive terms is good to about 1e-13
relative, 1e-10 leaves room for the square root and the order of summation; with the singular-value gaps the generator
guarantees (>= 1e-3) first-order perturbation theory puts a first update's error near 1e-13, bound 1e-9.  A full run is
discrete -- a correspondence that flips at rounding level can send a pair to another fixed point -- so there the bound is
a count of pairs: at most 1 in 16 may differ in (count, iters), which the fp64 restatement with a permuted summation order
stays well inside (at most 1 of 96 over three seeds) and an fp32 shortcut sits close to (at most 3 of 96)."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import splitter_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(GOLDEN, 'splitter.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _run(dev, src, tgt, it):
    from sug_amd import ops
    out = ops.icp_fitness(torch.from_numpy(np.ascontiguousarray(src)).to(dev), torch.from_numpy(np.ascontiguousarray(tgt)).to(dev),
                          max_iteration=it)
    return dict(zip(('count', 'rmse', 'iters', 'transform'), out))


@pytest.fixture(scope='module')
def runs(fx, dev):
    """Every pair set at every iteration setting, launched once: {(set, max_iteration): {name: numpy array}}."""
    out = {}
    for name in C.PAIR_SETS:
        src, tgt = C.pairs_of(fx, name)
        for it in C.ITER_SETTINGS:
            out[name, it] = {k: v.cpu().numpy() for k, v in _run(dev, src, tgt, it).items()}
    return out


def _ref(fx, name, it):
    return {k: fx['%s_it%d_%s' % (name, it, k)] for k in ('count', 'rmse', 'iters', 'transform')}


@pytest.mark.parametrize('name', list(C.PAIR_SETS))
def test_evaluation_only(fx, runs, name):
    got, ref = runs[name, 0], _ref(fx, name, 0)
    assert got['count'].dtype == np.int32 and got['rmse'].dtype == np.float64 and got['transform'].shape[1:] == (4, 4)
    err = np.abs(got['rmse'] - ref['rmse'])
    rel = err[ref['rmse'] > 0] / ref['rmse'][ref['rmse'] > 0]         # the anchor against itself has rmse 0 on both sides
    print('%s: counts %s, largest relative rmse error %.2e' % (name, got['count'].tolist(), rel.max()))
    assert np.array_equal(got['count'], ref['count'])
    assert (err <= 1e-10 * ref['rmse']).all()
    assert (got['iters'] == 0).all()
    assert np.array_equal(got['transform'], np.broadcast_to(np.eye(4), got['transform'].shape))


@pytest.mark.parametrize('name', list(C.PAIR_SETS))
def test_one_update(fx, runs, name):
    got, ref = runs[name, 1], _ref(fx, name, 1)
    T = got['transform']
    err = np.abs(T - ref['transform']).max()
    R = T[:, :3, :3]
    orth = np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).sum(axis=2).max()        # the infinity norm: largest row sum
    print('%s: transform error %.2e, |R^T R - I|_inf %.2e, counts %s' % (name, err, orth, got['count'].tolist()))
    assert err <= 1e-9
    assert orth <= 1e-12 and (np.linalg.det(R) > 0).all()
    assert np.array_equal(T[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], T[:, 3].shape))
    assert (got['iters'] == 1).all()
    assert np.array_equal(got['count'], ref['count'])


def _differing(got, ref, name):
    differ = np.flatnonzero((got['count'] != ref['count']) | (got['iters'] != ref['iters']))
    for b in differ:
        print('%s pair %d: count %d iters %d, the restatement has count %d iters %d'
              % (name, b, got['count'][b], got['iters'][b], ref['count'][b], ref['iters'][b]))
    agree = np.setdiff1d(np.arange(len(ref['count'])), differ)
    worst = np.abs(got['rmse'][agree] - ref['rmse'][agree]).max() if len(agree) else 0.0
    print('%s: %d of %d pairs differ %s; on the others the largest rmse difference is %.2e, iterations %s'
          % (name, len(differ), len(ref['count']), differ.tolist(), worst, np.bincount(got['iters']).tolist()))
    return differ, worst


def test_full_run_class(fx, runs):
    differ, worst = _differing(runs['cls', 30], _ref(fx, 'cls', 30), 'cls')
    assert len(differ) <= 6                              # at least 90 of the 96 pairs
    assert worst <= 1e-6                                 # the loop's own stopping scale


def test_full_run_500(fx, runs):
    differ, worst = _differing(runs['big', 30], _ref(fx, 'big', 30), 'big')
    assert len(differ) <= 1                              # they may not both differ
    assert worst <= 1e-6


def test_deterministic_and_batch_independent(fx, runs, dev):
    src, tgt = C.pairs_of(fx, 'cls')
    again = {k: v.cpu().numpy() for k, v in _run(dev, src, tgt, 30).items()}
    for k, v in again.items():
        assert np.array_equal(v, runs['cls', 30][k]), k
    alone = _run(dev, src, tgt[17:18], 30)               # one pair alone == the same pair inside the batch of 96
    for k, v in alone.items():
        assert np.array_equal(v.cpu().numpy(), again[k][17:18]), k
    rep = _run(dev, np.broadcast_to(src, (len(tgt),) + src.shape), tgt, 30)      # stride 3*Ns == stride 0
    for k, v in rep.items():
        assert np.array_equal(v.cpu().numpy(), again[k]), k
    bsrc, btgt = C.pairs_of(fx, 'big')
    for k, v in _run(dev, bsrc, btgt, 30).items():
        assert np.array_equal(v.cpu().numpy(), runs['big', 30][k]), k


def test_rank_deficient_update_is_a_finite_rotation(fx, dev):
    """The thin cylinder finds a handful of correspondences or none: outside the ground the restatement pins, where the
    kernel still has to return a proper rotation and no NaN."""
    first = _run(dev, fx['thin'], fx['clouds'], 0)['count'].cpu().numpy()
    assert (first == 0).any() and (first == 1).any() and (first == 2).any()      # what the first update starts from
    for it in (1, 30):
        out = {k: v.cpu().numpy() for k, v in _run(dev, fx['thin'], fx['clouds'], it).items()}
        assert np.array_equal(out['iters'] == 0, first == 0)
        assert all(np.isfinite(v).all() for v in out.values())
        R = out['transform'][:, :3, :3]
        assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).sum(axis=2).max() <= 1e-12 and (np.linalg.det(R) > 0).all()
    # a single correspondence: Sigma = 0, a pure translation onto the target point
    src = torch.tensor([[0.0, 0.0, 0.0], [5.0, 5.0, 5.0]], device=dev)
    tgt = torch.tensor([[[0.05, -0.03, 0.02], [-7.0, 0.0, 0.0]]], device=dev)
    from sug_amd import ops
    count, rmse, iters, T = ops.icp_fitness(src, tgt, max_iteration=1)
    assert count.item() == 1 and iters.item() == 1 and rmse.item() < 1e-15
    want = np.eye(4)
    want[:3, 3] = tgt[0, 0].double().cpu().numpy()
    assert np.array_equal(T[0].cpu().numpy(), want)


def test_process_pts(fx, dev):
    from sug_amd.dataset_splitter import process_pts
    pts, idx = process_pts(torch.from_numpy(fx['process_raw']).to(dev), C.PROCESS_N, return_index=True)
    assert pts.shape == (C.PROCESS_M, C.PROCESS_N, 3) and pts.dtype == torch.float32
    assert np.array_equal(idx.cpu().numpy(), fx['process_idx'])
    err = np.abs(pts.double().cpu().numpy() - fx['process_pts']).max()
    print('process_pts: largest coordinate error %.2e' % err)
    assert err <= 1e-6
    assert torch.equal(process_pts(torch.from_numpy(fx['process_raw']).to(dev), C.PROCESS_N), pts)
    with pytest.raises(ValueError, match='pt_num'):
        process_pts(torch.from_numpy(fx['process_raw']).to(dev), C.PROCESS_P + 1)


def _flips(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


@pytest.mark.parametrize('use_hist', [False, True])
def test_split_dataset_geometric(fx, dev, use_hist):
    from sug_amd import dataset_splitter as S
    tag = 'hist' if use_hist else 'mean'
    clouds = torch.from_numpy(fx['clouds']).to(dev)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        split = S.split_dataset_geometric(clouds, np.zeros(len(clouds), dtype=np.int64), use_hist=use_hist, num_class=1,
                                          anchors=[list(C.SPLIT_ANCHORS)], pt_num=C.N_PTS)
    assert split.tries == [int(fx['split_%s_tries' % tag])]
    assert len(caught) == (1 if use_hist else 0)              # the histogram cut refuses all five anchors: kept, with a warning
    assert split.anchors == [C.SPLIT_ANCHORS[split.tries[0] - 1]]
    assert np.array_equal(split.indices[0].cpu().numpy(), fx['split_%s_order' % tag])
    d = split.distances[0].cpu().numpy()
    labels = split.cluster_labels[0].cpu().numpy()
    assert np.array_equal(labels, C.split_rule(d, use_hist)[0])               # the rule, on the device's own distances
    flips = _flips(labels, fx['split_%s_labels' % tag])
    print('%s cut: %d zeros, %d labels differ from the restatement, %d distances differ'
          % (tag, (labels == 0).sum(), flips, _flips(d, fx['split_%s_dist' % tag])))
    assert flips <= 6                                                           # 1 in 16 of the 96
    # icp_distance on the processed clouds is what the split used
    processed = S.process_pts(clouds.index_select(0, split.indices[0]), C.N_PTS)
    assert np.array_equal(S.icp_distance(processed[split.anchors[0]], processed).cpu().numpy(), d)
    assert S.icp_distance(processed[split.anchors[0]], processed[3]).item() == d[3]


def test_split_redraw_and_subsets(fx, dev):
    from sug_amd import dataset_splitter as S
    from sug_amd.data.dataloader import UnifiedPointDG
    raw, anchors = C.redraw_class(fx)
    assert list(anchors) == fx['redraw_anchors'].tolist()
    # two classes: the redraw class (first anchor fails the balance test) and the first 24 clouds
    pts = torch.from_numpy(np.concatenate((raw, fx['clouds'][:24]))).to(dev)
    labels = np.array([0] * len(raw) + [1] * 24)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        split = S.split_dataset_geometric(pts, labels, num_class=2, anchors=[list(anchors), [7]], pt_num=C.N_PTS)
    assert split.tries == [2, 1] and split.anchors == [anchors[1], 7]
    for c in (0, 1):
        assert np.array_equal(split.cluster_labels[c].cpu().numpy(), C.split_rule(split.distances[c].cpu().numpy())[0])
    assert _flips(split.cluster_labels[0].cpu().numpy(), fx['redraw_labels']) <= 1           # 1 in 16 of the 21
    n0 = [int((split.cluster_labels[c] == 0).sum()) for c in (0, 1)]
    parts = S.as_dataset_spliter(pts, labels, split, swap=[False, True])
    assert parts['subset_1']['pts'].shape == (n0[0] + 24 - n0[1], C.N_PTS, 3)
    assert parts['subset_2']['pts'].shape == (len(raw) - n0[0] + n0[1], C.N_PTS, 3)
    assert parts['subset_1']['label'].tolist() == [0] * n0[0] + [1] * (24 - n0[1])
    full = S.as_dataset_spliter(pts, labels, split, subset_fullsize=True)
    assert full['subset_2']['pts'].shape[0] == len(pts) and full['subset_1']['pts'].shape[0] == sum(n0)
    first = split.indices[0][split.cluster_labels[0] == 0]
    assert torch.equal(full['subset_1']['pts'][:n0[0]], pts[first])
    # swap together with subset_fullsize, through the dictionary: every row of both subsets
    idx, cl = split.indices, split.cluster_labels
    one = torch.cat((idx[0][cl[0] == 0], idx[1][cl[1] == 1]))
    two = torch.cat((idx[0][cl[0] == 0], idx[0][cl[0] == 1], idx[1][cl[1] == 1], idx[1][cl[1] == 0]))
    both = S.as_dataset_spliter(pts, labels, split, swap=[False, True], subset_fullsize=True)
    lab = torch.as_tensor(labels, device=dev)
    for name, want in (('subset_1', one), ('subset_2', two)):
        assert torch.equal(both[name]['pts'], pts[want]) and torch.equal(both[name]['label'], lab[want]), name
    assert sorted(two.tolist()) == list(range(len(pts)))
    # what create_splitted_dataset does with the dictionary
    sets = [UnifiedPointDG('modelnet', parts[k]['pts'], parts[k]['label'], pc_input_num=C.N_PTS, aug=False) for k in parts]
    data, label = sets[0].batch([0, n0[0]])
    assert data.shape == (2, 3, C.N_PTS, 1) and label.tolist() == [0, 1]
    # a generator draws from arange(n // 4, n // 2) of the sorted order
    g = S.split_dataset_geometric(pts, labels, num_class=2, generator=np.random.default_rng(5), pt_num=C.N_PTS)
    assert 24 // 4 <= g.anchors[1] < 24 // 2 and len(raw) // 4 <= g.anchors[0] < len(raw) // 2


def test_entropy_clustering_quirks(dev):
    """A hand-made vector: entropies 0, ln 2, ln 4 and two in between.  With 4 bins ln 2 sits ON the third edge (ln 4 / 2)
    and belongs to bin 2; the maximum lies in no half-open bin and keeps the initial label 1; the minimum takes 0."""
    from sug_amd.dataset_splitter import entropy_clustering
    rows = [[1, 0, 0, 0], [0.5, 0.5, 0, 0], [0.25, 0.25, 0.25, 0.25], [0.9, 0.1, 0, 0], [0.4, 0.3, 0.2, 0.1]]
    probs = torch.tensor(rows, dtype=torch.float32, device=dev)
    labels, u = entropy_clustering(probs, cluster_num=4)
    un = u.cpu().numpy()
    np.testing.assert_allclose(un, C.entropy_clustering(np.array(rows), 4)[1], rtol=0, atol=1e-6)
    print('hand-made entropies %s, labels %s' % (un.tolist(), labels.tolist()))
    assert un[0] == 0 and 2 * un[1] == un[2]               # 0.5 log 0.5 + 0.5 log 0.5 and 4 x 0.25 log 0.25: the edge is hit exactly
    assert labels.tolist() == [0, 2, 1, 0, 3]
    assert entropy_clustering(probs, cluster_num=2)[0].tolist() == [0, 1, 1, 0, 1]
    # the reference's own lines on the device's entropies give the device's labels
    ref = np.ones(len(un))
    edges = np.histogram(un, bins=4)[1]
    for i in range(4):
        ref[np.where((un >= edges[i]) & (un < edges[i + 1]))] = i
    assert labels.tolist() == ref.astype(int).tolist()


@pytest.mark.parametrize('cluster_num', [2, 4])
def test_entropy_clustering(fx, dev, cluster_num):
    from sug_amd.dataset_splitter import entropy_clustering
    labels, u = entropy_clustering(torch.from_numpy(fx['probs']).to(dev), cluster_num)
    assert labels.dtype == torch.int64 and labels.is_cuda and u.is_cuda and len(fx['probs']) == C.ENT_ROWS
    err = np.abs(u.double().cpu().numpy() - fx['ent_u']).max()
    print('entropy: largest error %.2e, bins %s' % (err, np.bincount(labels.cpu().numpy()).tolist()))
    assert err <= 1e-6
    assert np.array_equal(labels.cpu().numpy(), fx['ent_labels_%d' % cluster_num])
