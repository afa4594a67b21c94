"""CPU: the variance / ratio estimator and the linear-time estimators of sug_amd.model.mmd -- the coefficient formulas of
the HIP coefficient kernel restated in fp64 against autograd, the mirror's names and signatures, the header / ctypes /
Python limits, the host-side limit checks of the four entry points, and the composed lines against the reference's fp64
results recorded in tests/golden/mmd_estimators.npz."""
import ctypes
import inspect
import re

import pytest
import torch

import mmd_estimator_cases as C


@pytest.mark.parametrize('m', [2, 3, 7])
def test_variance_partials_equal_autograd_of_the_formula(m):
    """m = 2 and 3: the factors m - 2 and m - 3 vanish or change sign."""
    from sug_amd.model import mmd
    g = torch.Generator().manual_seed(m)
    K = [(torch.rand(m, m, generator=g, dtype=torch.float64) + 0.1).requires_grad_(True) for _ in range(3)]
    _, var = mmd._mmd2_and_variance(*K, biased=False)
    want = torch.autograd.grad(var, K)
    got = C.variance_partials(*(k.detach() for k in K))
    for w, h, name in zip(want, got, ('K_XX', 'K_XY', 'K_YY')):
        scale = float(w.abs().max())
        assert float((w - h).abs().max()) <= 1e-14 * max(scale, 1.0), name
    assert not want[0].diagonal().any() and not want[2].diagonal().any()


def test_mirror_has_the_reference_names_and_signatures():
    from sug_amd.model import mmd
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(mmd.mix_rbf_mmd2_and_ratio) == [('X', E), ('Y', E), ('sigma_list', E), ('biased', True)]
    assert sig(mmd.linear_mmd2) == [('f_of_X', E), ('f_of_Y', E)]
    assert sig(mmd.poly_mmd2) == [('f_of_X', E), ('f_of_Y', E), ('d', 2), ('alpha', 1.0), ('c', 2.0)]


def test_header_ctypes_table_and_python_limits_agree():
    from sug_amd import _lib, ops
    H = _lib.CONSTANTS
    assert (ops.MMD_EST_MAX_ROWS, ops.MMD_EST_MAX_D, ops.MMD_EST_MAX_SIGMAS, ops.MMD_POLY_MAX_DEGREE) == \
        (H['SUG_MMD_EST_MAX_ROWS'], H['SUG_MMD_EST_MAX_D'], H['SUG_MMD_EST_MAX_SIGMAS'], H['SUG_MMD_POLY_MAX_DEGREE']) == \
        (1024, 1 << 20, 8, 8)
    assert (H['SUG_MMD_RATIO_ROW_FIELDS'], H['SUG_MMD_RATIO_STATS'], H['SUG_ABI_VERSION']) == (9, 16, 8)
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    want = {
        'sug_mmd_ratio_fwd': [vp, i64, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        'sug_mmd_ratio_bwd': [vp, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp],
        'sug_mmd_adjacent_fwd': [vp, i64, vp, i64, i32, i32, i32, i32, f64, f64, vp, vp, vp, vp],
        'sug_mmd_adjacent_bwd': [vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, i64, vp, i64, vp],
    }
    L = _lib.lib()
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == args, name
        assert getattr(L, name).argtypes == args


def _refused(rc, what):
    from sug_amd import _lib
    msg = _lib.lib().sug_last_error().decode()
    assert rc == -1 and re.search(what, msg), (rc, msg)


def test_limits_are_checked_on_the_host_and_name_the_argument():
    """One past each limit (and m = 1): refused before any launch, the message names the entry point, the argument, its value
    and the limit.  The buffers are host memory; nothing reads them."""
    from sug_amd import _lib
    L, H = _lib.lib(), _lib.CONSTANTS
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    M, DM, NS, DEG = (H['SUG_MMD_' + k] for k in ('EST_MAX_ROWS', 'EST_MAX_D', 'EST_MAX_SIGMAS', 'POLY_MAX_DEGREE'))
    fwd = lambda m, D, ns: L.sug_mmd_ratio_fwd(p, D, m, D, p, ns, 1, p, p, p, p, p, p, p, None)
    for m in (1, 0, M + 1):
        _refused(fwd(m, 8, 5), r'sug_mmd_ratio_fwd: m=%d\b.*\b%d\b' % (m, M))
    for D in (0, DM + 1):
        _refused(fwd(8, D, 5), r'sug_mmd_ratio_fwd: D=%d\b.*\b%d\b' % (D, DM))
    for ns in (0, NS + 1):
        _refused(fwd(8, 8, ns), r'sug_mmd_ratio_fwd: nsigma=%d\b.*\b%d\b' % (ns, NS))
    _refused(L.sug_mmd_ratio_fwd(p, 7, 8, 8, p, 5, 1, p, p, p, p, p, p, p, None), r'sug_mmd_ratio_fwd: row stride 7 < D=8')
    _refused(L.sug_mmd_ratio_fwd(p, 8, 8, 8, p, 5, 1, p, p, p, p, p, p, None, None), r'wt_m and wt_v')
    _refused(L.sug_mmd_ratio_bwd(p, 8, 1, 8, p, p, p, p, p, 8, None), r'sug_mmd_ratio_bwd: m=1\b')
    _refused(L.sug_mmd_ratio_bwd(p, 8, 8, 8, p, p, p, p, p, 7, None), r'sug_mmd_ratio_bwd: row stride 7 < D=8')
    adj = lambda m, D, mode, deg: L.sug_mmd_adjacent_fwd(p, D, p, D, m, D, mode, deg, 1.0, 2.0, p, p, p, None)
    _refused(adj(1, 8, 0, 1), r'sug_mmd_adjacent_fwd: m=1\b')
    _refused(adj(M + 1, 8, 1, 2), r'sug_mmd_adjacent_fwd: m=%d\b' % (M + 1))
    _refused(adj(8, DM + 1, 1, 2), r'sug_mmd_adjacent_fwd: D=%d\b' % (DM + 1))
    for deg in (0, DEG + 1):
        _refused(adj(8, 8, 1, deg), r'sug_mmd_adjacent_fwd: degree=%d\b.*\b%d\b' % (deg, DEG))
    _refused(adj(8, 8, 2, 2), r'sug_mmd_adjacent_fwd: mode 2')
    _refused(L.sug_mmd_adjacent_bwd(p, 8, p, 8, 1, 8, 0, p, p, p, 8, p, 8, None), r'sug_mmd_adjacent_bwd: m=1\b')
    _refused(L.sug_mmd_adjacent_bwd(p, 8, p, 8, 8, 8, 1, None, p, p, 8, p, 8, None), r'sug_mmd_adjacent_bwd: null')


def test_composed_lines_reproduce_the_recorded_reference_in_fp64():
    """The fp64 references of the GPU tests come from the mirror's composed lines on the CPU: their values are the
    reference's, recorded when the fixture was made (which also compared the gradients)."""
    G = C.golden()
    for ci in range(len(C.ratio_case_ids())):
        for b in (0, 1):
            out, _ = C.ratio_ref64(ci, b)
            want = G['r%d_b%d_out64' % (ci, b)]
            assert float((out - want).abs().max()) <= 1e-11 * float(want.abs().max()), (ci, b)
    for si in range(G['adj_shapes'].shape[0]):
        for pi in range(len(C.adjacent_params())):
            v, _ = C.adjacent_ref64(si, pi)
            want = G['a%d_p%d_v64' % (si, pi)]
            assert abs(float(v - want)) <= 1e-11 * max(abs(float(want)), 1e-300), (si, pi)


def test_fixture_keeps_clear_of_the_clamp_and_has_both_outcomes():
    G = C.golden()
    var = [float(G['r%d_b%d_out64' % (ci, b)][2]) for ci in range(len(C.ratio_case_ids())) for b in (0, 1)]
    assert all(v <= 0 or v >= 1e-6 for v in var)
    assert any(v <= 0 for v in var) and any(v >= 1e-6 for v in var)


def test_one_row_per_domain_and_cpu_tensors_take_the_composed_lines():
    """m = 1 as the reference has it (recorded in the fixture): the linear-time estimators average nothing (NaN), the ratio
    estimator divides by m - 1 = 0 in Python.  ops.mmd_ratio refuses m = 1 before any launch."""
    from sug_amd import ops
    from sug_amd.model import mmd
    X, Y = torch.randn(1, 4), torch.randn(1, 4)
    assert torch.isnan(mmd.linear_mmd2(X, Y)) and torch.isnan(mmd.poly_mmd2(X, Y))
    assert C.golden()['ratio_one_row'] == ['ZeroDivisionError']
    with pytest.raises(ZeroDivisionError):
        mmd.mix_rbf_mmd2_and_ratio(X, Y, mmd.sigma_list)
    with pytest.raises(RuntimeError, match='m=1'):
        ops.mmd_ratio(torch.cat((X, Y), 0), 1)
    X, Y = torch.randn(4, 6), torch.randn(4, 6)
    assert not ops.mmd_ratio_supported(X, Y) and not ops.adjacent_mmd_supported(X, Y)
    with pytest.raises(RuntimeError):
        ops.linear_mmd2(X, Y)
    loss, mmd2, var = mmd.mix_rbf_mmd2_and_ratio(X, Y, mmd.sigma_list, biased=False)
    assert float(loss) == float(mmd2 / torch.sqrt(torch.clamp(var, min=1e-8)))
