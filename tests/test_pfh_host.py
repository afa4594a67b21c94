"""CPU: the PFH feature's host side -- the numpy restatement (tests/pfh_cases.py) against the fixture the reference wrote
(tests/golden/pfh.npz, tests/golden/make_pfh_goldens.py), the ABI entries and their host-side refusals, what is not mirrored.

Bounds: the fixture keeps every discrete decision at least 1e-9 away from flipping, so counts and neighbour lists are asked
for EXACTLY.  A normal is the eigenvector of a covariance whose rounding error is a few 2^-52 of its norm; first-order
perturbation theory divides that by the relative eigen gap: 64 * 2^-52 / gap per point.  A distance is the square root of a
sum of D squares of exact differences of multiples of 1/36: (D + 2) * 2^-52 relative covers every summation order."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import pfh_cases as C


@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(GOLDEN, 'pfh.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def restated(fx):
    return {name: C.descriptors(fx[name + '_pts'], rad, k, div) for name, (N, rad, div, k) in C.CASES.items()}


def test_fixture_shapes_and_size(fx):
    assert os.path.getsize(os.path.join(GOLDEN, 'pfh.npz')) < 200 * 1000
    for name, (N, rad, div, k) in C.CASES.items():
        assert fx[name + '_pts'].shape == (N, 3) and fx[name + '_pts'].dtype == np.float32
        assert fx[name + '_counts'].shape == (N, div ** 3) and fx[name + '_counts'].dtype == np.uint8
        assert fx[name + '_normals'].shape == (N, 3) and fx[name + '_nbr'].shape == (N, k)
        assert fx[name + '_gap'].min() >= C.GAP
        cnt = (fx[name + '_nbr'] >= 0).sum(axis=1)
        assert cnt.min() >= 3 and np.array_equal(fx[name + '_counts'].sum(axis=1), (cnt + 1) * cnt // 2)
    assert ((fx['n9_d2_nbr'] >= 0).sum(axis=1) == 8).all()
    assert np.array_equal(fx['c500_d5_pts'], fx['c500_d2_pts'])


@pytest.mark.parametrize('name', list(C.CASES))
def test_restatement_reproduces_the_reference(fx, restated, name):
    r = restated[name]
    N, rad, div, k = C.CASES[name]
    assert r['margin'] >= C.MARGIN and r['used_cnt'] == N
    assert np.array_equal(r['idx'], fx[name + '_nbr'])
    assert np.array_equal(r['counts'], fx[name + '_counts'])
    err = np.abs(r['normals'] - fx[name + '_normals']).max(axis=1)
    print('%s: largest normal error %.2e, in units of its bound %.3f' % (name, err.max(), (err / C.normal_bound(r['gap'])).max()))
    assert (err <= C.normal_bound(r['gap'])).all()
    np.testing.assert_allclose(r['gap'], fx[name + '_gap'], rtol=1e-9)


def test_restatement_reproduces_the_distances(fx, restated):
    keys = [k for k in fx if k.startswith('dist_')]
    assert len(keys) == 18
    for key in keys:
        s, t = key[len('dist_'):].split('__')
        D = C.CASES[s][2] ** 3
        used_s, used_t = restated[s]['cnt'] > 0, restated[t]['cnt'] > 0
        got, ref = C.hist_distance(restated[s]['hist'], used_s, restated[t]['hist'], used_t), float(fx[key])
        assert abs(got - ref) <= C.distance_bound(D) * ref, key
        if s == t:
            assert got == 0.0 and ref == 0.0


def test_restatement_unused_points_and_median():
    P = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0.1, 0.1, 0.05], [5, 5, 5]], dtype=np.float32)
    r = C.descriptors(P, 0.3, 8, 2)
    assert r['cnt'].tolist() == [3, 3, 3, 3, 0] and r['used_cnt'] == 4
    assert not r['counts'][4].any() and not r['normals'][4].any() and (r['idx'][4] == -1).all()
    assert r['counts'][:4].sum(axis=1).tolist() == [6, 6, 6, 6]                  # comb(4, 2) pairs, of comb(9, 2) = 36
    h = np.array([[0.0, 0], [1, 0], [3, 0], [6, 0]])
    t = np.zeros((1, 2))
    assert C.hist_distance(h, [1, 1, 1, 1], t, [1]) == 2.0                       # even: the mean of 1 and 3
    assert C.hist_distance(h, [1, 1, 1, 0], t, [1]) == 1.0                       # odd
    assert np.isnan(C.hist_distance(h, [0, 0, 0, 0], t, [1])) and np.isnan(C.hist_distance(h, [1, 1, 1, 1], t, [0]))
    # an exact duplicate of lower index: the duplicate is dropped, the point stays its own neighbour
    Q = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], dtype=np.float32)
    idx, cnt, _ = C.neighbours(Q.astype(np.float64), 0.5, 8)
    assert idx[:, 0].tolist() == [1, 1, -1] and cnt.tolist() == [1, 1, 0]


# ----------------------------------------------------------------------------------------------------------- ABI
def test_header_constants_and_bindings():
    from sug_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'sug_amd.h')).read()
    assert 'int sug_pfh_descriptors(const float* pts, int M, int N, double rad, int nneighbors, int div,' in header
    assert 'int sug_pfh_hist_distance(const double* histS, const int32_t* cntS, int64_t src_batch_stride,' in header
    H = _lib.CONSTANTS
    assert (H['SUG_PFH_MAX_POINTS'], H['SUG_PFH_MAX_NEIGHBORS'], H['SUG_ABI_VERSION']) == (1024, 16, 8)
    assert (ops.PFH_MAX_POINTS, ops.PFH_MAX_NEIGHBORS) == (1024, 16)
    P, I, L, Dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    assert _lib.DECLARATIONS['sug_pfh_descriptors'] == (I, [P, I, I, Dbl, I, I, P, P, P, P, P, P])
    assert _lib.DECLARATIONS['sug_pfh_hist_distance'] == (I, [P, P, L, P, P, I, I, I, I, P, P])
    for name in ('sug_pfh_descriptors', 'sug_pfh_hist_distance'):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_descriptor_refusals_before_any_launch():
    """Argument validation happens on the host before the launch: safe without a GPU."""
    from sug_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)

    def call(pts=p, M=1, N=8, rad=0.2, k=8, div=2, hist=p, normals=p, idx=p, cnt=p, used=p):
        return L.sug_pfh_descriptors(pts, M, N, rad, k, div, hist, normals, idx, cnt, used, None)
    assert call(N=0) == -1 and b'N=0' in L.sug_last_error()
    assert call(N=1025) == -1 and b'N=1025' in L.sug_last_error() and b'1024' in L.sug_last_error()
    assert call(k=0) == -1 and b'nneighbors=0' in L.sug_last_error()
    assert call(k=17) == -1 and b'nneighbors=17' in L.sug_last_error()
    assert call(div=1) == -1 and b'div=1' in L.sug_last_error()
    assert call(div=6) == -1 and b'div=6' in L.sug_last_error()
    for name in ('pts', 'hist', 'normals', 'idx', 'cnt', 'used'):
        assert call(**{name: None}) == -1 and b'null' in L.sug_last_error(), name
    assert call(M=0) == -1 and b'M=0' in L.sug_last_error()
    for rad in (0.0, -1.0, float('inf'), float('nan')):
        assert call(rad=rad) == -1 and b'rad=' in L.sug_last_error()


def test_distance_refusals_before_any_launch():
    from sug_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)

    def call(hs=p, cs=p, stride=0, ht=p, ct=p, B=1, Ns=8, Nt=8, D=8, out=p):
        return L.sug_pfh_hist_distance(hs, cs, stride, ht, ct, B, Ns, Nt, D, out, None)
    assert call(Ns=0) == -1 and b'Ns=0' in L.sug_last_error()
    assert call(Nt=1025) == -1 and b'Nt=1025' in L.sug_last_error()
    assert call(Ns=1025) == -1 and call(Nt=0) == -1 and call(B=0) == -1
    assert call(D=1) == -1 and b'D=1' in L.sug_last_error()                       # div = 1
    assert call(D=216) == -1 and b'D=216' in L.sug_last_error()                   # div = 6
    assert call(D=9) == -1
    for name in ('hs', 'cs', 'ht', 'ct', 'out'):
        assert call(**{name: None}) == -1 and b'null' in L.sug_last_error(), name
    assert call(stride=5) == -1 and b'src_batch_stride=5' in L.sug_last_error()
    assert call(stride=8) == -1                                                   # Ns, not Ns * D


# ------------------------------------------------------------------------------------------------ the Python layer
def test_not_mirrored_classes_raise():
    from sug_amd.utils import pfh
    x = torch.zeros(8, 3)
    with pytest.raises(NotImplementedError, match='SPFH'):
        pfh.SPFH(0.1, 2, 8, 0.2).calcHistArray(x, None, None)
    with pytest.raises(NotImplementedError, match='FPFH'):
        pfh.FPFH(0.1, 2, 8, 0.2).calcHistArray(x, None, None)
    with pytest.raises(NotImplementedError, match='solve'):
        pfh.PFH(0.1, 2, 8, 0.2).solve(x, x)
    with pytest.raises(NotImplementedError, match='only PFH'):
        pfh.get_pfh_descriptor(torch.zeros(2, 8, 3), method='FPFH')
    with pytest.raises(ValueError, match='div'):
        pfh.PFH(0.1, 6, 8, 0.2)
    with pytest.raises(ValueError, match='nneighbors'):
        pfh.PFH(0.1, 2, 17, 0.2)


def test_thresholds_are_the_references():
    from sug_amd.utils import pfh
    for div in (2, 3, 4, 5):
        s = pfh.PFH(0.1, div, 8, 0.2).calc_thresholds()
        assert s.shape == (3, div - 1) and np.array_equal(s, C.thresholds(div))
    assert pfh.PFH(0.1, 2, 8, 0.2).calc_thresholds().tolist() == [[0.0], [0.0], [0.0]]


def test_cpu_tensors_raise():
    from sug_amd import dataset_splitter as S, ops
    from sug_amd.utils import pfh
    pts = torch.zeros(2, 16, 3)
    h, c = torch.zeros(2, 16, 8, dtype=torch.float64), torch.zeros(2, 16, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.pfh_descriptors(pts)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.pfh_hist_distance(h[0], c[0], h, c)
    with pytest.raises(RuntimeError, match='HIP device'):
        pfh.PFH(0.1, 2, 8, 0.2).calc_normals(pts)
    with pytest.raises(RuntimeError, match='HIP device'):
        pfh.PFH(0.1, 2, 8, 0.2).calcHistArray(pts[0])
    with pytest.raises(RuntimeError, match='HIP device'):
        pfh.get_pfh_descriptor(pts)
    with pytest.raises(RuntimeError, match='HIP device'):
        pfh.pfh_hist_distance(h[0], h)
    with pytest.raises(RuntimeError, match='HIP device'):
        pfh.process_pts(pts, 8)
    with pytest.raises(RuntimeError, match='HIP device'):
        S.split_dataset_geometric(torch.zeros(40, 16, 3), np.arange(40) % 10, metric='pfh')
    with pytest.raises(ValueError, match='metric'):
        S.split_dataset_geometric(torch.zeros(40, 16, 3), np.arange(40) % 10, metric='chamfer')
