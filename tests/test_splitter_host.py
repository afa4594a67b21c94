"""CPU: the sub-domain splitter's host side -- the fixture against the restatement that made it, the split rule and the
anchor loop on injected distances, the subset assembly, the entropy quirks, the ABI entry and its host-side refusals."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import splitter_cases as C


@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(GOLDEN, 'splitter.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------- fixture <-> restatement
def test_fixture_inputs_come_from_the_seeds(fx):
    for k, v in C.inputs().items():
        assert fx[k].dtype == v.dtype and fx[k].shape == v.shape, k
        np.testing.assert_allclose(fx[k], v, rtol=0, atol=1e-6, err_msg=k)
    assert os.path.getsize(os.path.join(GOLDEN, 'splitter.npz')) < 200 * 1000


def test_restatement_reproduces_the_fixture(fx):
    """On the STORED inputs (so that a libm that differs in the last bit of a cosine cannot matter) the restatement gives
    the stored results: the discrete ones exactly, the real ones to 1e-12."""
    out = C.results(fx)
    assert set(out) <= set(fx)
    for k, v in out.items():
        if np.asarray(v).dtype.kind in 'iub':
            assert np.array_equal(fx[k], v), k
        else:
            np.testing.assert_allclose(fx[k], v, rtol=0, atol=1e-12, err_msg=k)


def test_fixture_covers_what_the_gpu_tests_need(fx):
    assert fx['clouds'].shape == (96, 64, 3) and fx['odd_src'].shape == (8, 61, 3) and fx['odd_tgt'].shape == (8, 77, 3)
    assert fx['big_src'].shape == (2, 500, 3) and fx['big_tgt'].shape == (2, 500, 3)
    for name in C.PAIR_SETS:
        assert (fx[name + '_it0_iters'] == 0).all() and (fx[name + '_it1_iters'] == 1).all()
        assert np.array_equal(fx[name + '_it0_transform'], np.broadcast_to(np.eye(4), fx[name + '_it0_transform'].shape))
    it = fx['cls_it30_iters']
    assert it.min() >= 1 and it.max() < 30 and len(set(it.tolist())) > 5        # the loop stops by its criteria
    assert fx['split_mean_tries'] == 1 and fx['split_hist_tries'] == 5 and fx['redraw_tries'] == 2
    for tag in ('mean', 'hist'):
        assert sorted(fx['split_%s_order' % tag].tolist()) == list(range(96))
    assert 9 < (fx['split_mean_labels'] == 0).sum() < 87
    # the largest entropy keeps label 1 whatever the bin count, the smallest takes 0
    for k in (2, 4):
        assert fx['ent_labels_%d' % k][fx['ent_u'].argmax()] == 1 and fx['ent_labels_%d' % k][fx['ent_u'].argmin()] == 0
        assert set(fx['ent_labels_%d' % k].tolist()) == set(range(k))


# --------------------------------------------------------------------------------------------------- the split rule
def test_split_rule_thresholds():
    from sug_amd.dataset_splitter import _geometric_labels as geometric_labels
    d = np.array([0.0, 0.1, 0.2, 0.3, 0.9, 1.0, 0.35, 0.05])
    labels, ok = geometric_labels(d)                          # mean 0.3625
    assert labels.tolist() == [0, 0, 0, 0, 1, 1, 0, 0] and ok
    labels, ok = geometric_labels(d, use_hist=True)           # middle edge 0.5
    assert labels.tolist() == [0, 0, 0, 0, 1, 1, 0, 0] and ok
    d = np.array([0.0, 0.4, 0.45, 0.45, 0.45, 0.6, 0.6, 1.0])
    assert geometric_labels(d)[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]              # mean 0.49375
    assert geometric_labels(d, use_hist=True)[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    g = np.random.default_rng(0)
    for use_hist in (False, True):
        for _ in range(20):
            d = g.uniform(0, 1, 37) ** 3
            got, ref = geometric_labels(d, use_hist), C.split_rule(d, use_hist)
            assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]
    # a value equal to the threshold is NOT below it
    assert geometric_labels(np.array([0.25, 0.25, 0.25, 0.25]))[0].tolist() == [1, 1, 1, 1]


def test_split_rule_balance_test():
    from sug_amd.dataset_splitter import _geometric_labels as geometric_labels
    n = 20                                                    # accepted iff |n0 - 10| < 8, i.e. 3 <= n0 <= 17

    def with_zeros(n0):
        return np.concatenate((np.zeros(n0), np.ones(n - n0)))
    for n0, want in ((1, False), (2, False), (3, True), (10, True), (17, True), (18, False), (19, False)):
        labels, ok = geometric_labels(with_zeros(n0))
        assert ok == want and (labels == 0).sum() == n0, n0
    assert geometric_labels(np.full(n, 0.5))[1] is False      # nothing below the mean: n0 = 0


def test_anchor_loop_five_tries_then_keep():
    from sug_amd.dataset_splitter import _split_class as split_class
    n = 20
    bad = [np.concatenate((np.zeros(1), np.full(n - 1, 0.1 * (k + 1)))) for k in range(7)]
    good = np.concatenate((np.zeros(9), np.ones(n - 9)))
    # accepted on the third try: two redraws, no warning
    table = [bad[0], bad[1], good, bad[2]]
    draws = iter(range(4))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        labels, d, anchor, tries = split_class(n, lambda a: table[a], lambda: next(draws))
    assert tries == 3 and anchor == 2 and np.array_equal(d, good) and (labels == 0).sum() == 9
    # never accepted: exactly five tries, the fifth is kept, with a warning
    calls = []
    draws = iter(range(7))
    with pytest.warns(UserWarning, match='cannot find a suitable split'):
        labels, d, anchor, tries = split_class(n, lambda a: calls.append(a) or bad[a], lambda: next(draws))
    assert calls == [0, 1, 2, 3, 4] and tries == 5 and anchor == 4 and np.array_equal(d, bad[4])
    assert labels.tolist() == [0] + [1] * (n - 1)
    with pytest.raises(ValueError, match='outside'):
        split_class(n, lambda a: good, lambda: n)


def test_geometric_split_refusals():
    from sug_amd.dataset_splitter import split_dataset_geometric
    pts = torch.zeros(40, 16, 3)
    labels = np.arange(40) % 10
    with pytest.raises(ValueError, match='2 clusters'):
        split_dataset_geometric(pts, labels, cluster_num=4)
    with pytest.raises(ValueError, match='class 0 has 3 clouds'):
        split_dataset_geometric(pts[:39], np.concatenate((labels[:30], labels[31:])))
    with pytest.raises(ValueError, match='labels'):
        split_dataset_geometric(pts, labels[:5])


def test_cpu_tensors_raise():
    from sug_amd import dataset_splitter as S, ops
    pts = torch.zeros(40, 16, 3)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.icp_fitness(torch.zeros(8, 3), torch.zeros(2, 8, 3))
    with pytest.raises(RuntimeError, match='HIP device'):
        S.process_pts(pts, 8)
    with pytest.raises(RuntimeError, match='HIP device'):
        S.icp_distance(pts[0], pts)
    with pytest.raises(RuntimeError, match='HIP device'):
        S.split_dataset_geometric(pts, np.arange(40) % 10)
    with pytest.raises(RuntimeError, match='HIP device'):
        S.entropy_clustering(torch.full((4, 10), 0.1))
    split = S.GeometricSplit([torch.arange(4)], [torch.tensor([0, 1, 0, 1])], [None], [0], [1])
    with pytest.raises(RuntimeError, match='HIP device'):
        S.as_dataset_spliter(pts, np.zeros(40), split)


# ------------------------------------------------------------------------------------------------- subset assembly
def test_subset_indices_shapes_swap_and_fullsize():
    from sug_amd.dataset_splitter import _subset_indices as subset_indices
    idx = [torch.tensor([7, 3, 5, 1]), torch.tensor([0, 2, 4, 6, 8])]            # per class, in sorted order
    cl = [torch.tensor([0, 1, 0, 1]), torch.tensor([1, 1, 0, 1, 0])]
    one, two = subset_indices(idx, cl)
    assert one.tolist() == [7, 5, 4, 8] and two.tolist() == [3, 1, 0, 2, 6]
    one, two = subset_indices(idx, cl, swap=[True, False])
    assert one.tolist() == [3, 1, 4, 8] and two.tolist() == [7, 5, 0, 2, 6]
    one, two = subset_indices(idx, cl, swap=[False, True], subset_fullsize=True)
    assert one.tolist() == [7, 5, 0, 2, 6]
    assert two.tolist() == [7, 5, 3, 1, 0, 2, 6, 4, 8]                           # the whole class, subset_1's cluster first
    assert len(one) + len(subset_indices(idx, cl, swap=[False, True])[1]) == 9


# ------------------------------------------------------------------------------------------------------- entropy
def test_entropy_clustering_quirks_of_the_restatement():
    """A hand-made vector: entropies 0, ln 2, ln 4 and two in between."""
    rows = [[1, 0, 0, 0], [0.5, 0.5, 0, 0], [0.25, 0.25, 0.25, 0.25], [0.9, 0.1, 0, 0], [0.4, 0.3, 0.2, 0.1]]
    labels, u = C.entropy_clustering(np.array(rows), cluster_num=4)
    np.testing.assert_allclose(u, [0, np.log(2), np.log(4), 0.3250829733914482, 1.2798542258336676], atol=1e-12)
    # edges 0, ln4/4, ln4/2, 3 ln4/4, ln4: ln 2 sits ON the third edge (bin 2), the maximum is in no half-open bin: 1
    assert labels.tolist() == [0, 2, 1, 0, 3]
    labels, _ = C.entropy_clustering(np.array(rows), cluster_num=2)
    assert labels.tolist() == [0, 1, 1, 0, 1]


def test_histogram_edges_from_the_two_ends():
    """entropy_clustering on the device reads back the smallest and the largest entropy only: numpy's edges depend on
    nothing else, in fp32 as in fp64."""
    g = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        u = g.uniform(0, 2.3, 257).astype(dtype)
        for bins in (2, 4):
            full = np.histogram(u, bins=bins)[1]
            ends = np.histogram(np.array([u.min(), u.max()], dtype=dtype), bins=bins)[1]
            assert full.dtype == ends.dtype and np.array_equal(full, ends)


# ----------------------------------------------------------------------------------------------------------- ABI
def test_symbol_declared_and_bound():
    from sug_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'sug_amd.h')).read()
    assert 'int sug_icp_fitness(const float* src, int64_t src_batch_stride, const float* tgt, int B, int Ns, int Nt,' in header
    assert _lib.DECLARATIONS['sug_icp_fitness'][0] is ctypes.c_int and len(_lib.SIGNATURES['sug_icp_fitness']) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'sug_icp_fitness')
    assert not any(name.startswith('sug_icp') and name.endswith('workspace') for name in _lib.DECLARATIONS)


def test_host_side_refusals_before_any_launch():
    """Argument validation happens on the host before the launch: safe without a GPU."""
    from sug_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)

    def call(src=p, stride=0, tgt=p, B=1, Ns=8, Nt=8, r=0.15, it=30, count=p, rmse=p, iters=p, tf=p):
        return L.sug_icp_fitness(src, stride, tgt, B, Ns, Nt, r, it, 1e-6, 1e-6, count, rmse, iters, tf, None)
    assert call(Ns=1025) == -1 and b'1025' in L.sug_last_error()
    assert call(Nt=1025) == -1 and call(Ns=0) == -1 and call(Nt=0) == -1
    assert call(it=65) == -1 and b'max_iteration=65' in L.sug_last_error()
    assert call(it=-1) == -1
    for k in ('src', 'tgt', 'count', 'rmse', 'iters', 'tf'):
        assert call(**{k: None}) == -1 and b'null' in L.sug_last_error(), k
    assert call(r=0.0) == -1 and b'max_corr_dist' in L.sug_last_error()
    assert call(r=-1.0) == -1 and call(r=float('nan')) == -1
    assert call(stride=5) == -1 and b'src_batch_stride' in L.sug_last_error()
    assert call(B=0) == -1
