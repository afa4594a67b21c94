"""Shared by tests/test_mmd_estimators_host.py and tests/test_gpu_mmd_estimators.py: the cases of
tests/golden/mmd_estimators.npz, their fp64 references (computed once, on the CPU, with the composed lines of
sug_amd.model.mmd -- which make_mmd_estimator_goldens.py proved equal to the reference's functions in fp64, and whose fp64
values the fixture pins), and the fp64 restatement of the variance estimator's partial derivatives."""
import functools

import torch

from conftest import load_golden

SIGMAS = [0.01, 0.1, 1, 10, 100]
UPSTREAMS = ('loss', 'mmd2', 'var_est')


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden('mmd_estimators.npz')


def ratio_case_ids():
    return ['m%d-D%d-s%g' % (int(m), int(D), s) for m, D, s, _ in golden()['ratio_cases'].tolist()]


def ratio_inputs(ci):
    G = golden()
    return G['r%d_X' % ci].float(), G['r%d_Y' % ci].float()


def adjacent_inputs(si):
    G = golden()
    return G['a%d_X' % si].float(), G['a%d_Y' % si].float()


def adjacent_params():
    """[(d, alpha, c)]; d == 0 is linear_mmd2, an integer-valued d is an int as a caller would pass it."""
    return [(int(d) if float(d).is_integer() else d, a, c) for d, a, c in golden()['adj_params'].tolist()]


@functools.lru_cache(maxsize=None)
def ratio_ref64(ci, biased, sigmas=tuple(SIGMAS)):
    """(out64 [3], [grad64 [2m, D] per upstream]) of the composed lines on the CPU in fp64."""
    from sug_amd.model import mmd
    X, Y = (t.double().requires_grad_(True) for t in ratio_inputs(ci))
    out = mmd.mix_rbf_mmd2_and_ratio(X, Y, list(sigmas), biased=bool(biased))
    grads = [torch.cat(torch.autograd.grad(o, (X, Y), retain_graph=True), 0) for o in out]
    return torch.stack([o.detach() for o in out]), grads


def adjacent_call(mod, X, Y, d, alpha, c):
    return mod.linear_mmd2(X, Y) if d == 0 else mod.poly_mmd2(X, Y, d=d, alpha=alpha, c=c)


@functools.lru_cache(maxsize=None)
def adjacent_ref64(si, pi):
    from sug_amd.model import mmd
    X, Y = (t.double().requires_grad_(True) for t in adjacent_inputs(si))
    v = adjacent_call(mmd, X, Y, *adjacent_params()[pi])
    return v.detach(), torch.cat(torch.autograd.grad(v, (X, Y)), 0)


def variance_partials(K_XX, K_XY, K_YY):
    """d var_est / dK of _mmd2_and_variance (model/mmd.py:360-372) per entry of the three blocks, fp64, as the coefficient
    kernel forms them (before it symmetrises and multiplies by G): zero on the diagonals of K_XX and K_YY."""
    m = K_XX.shape[0]
    c1 = 2.0 / (m ** 2 * (m - 1) ** 2)
    c2 = (4.0 * m - 6.0) / (m ** 3 * (m - 1) ** 3)
    c3 = 4.0 * (m - 2) / (m ** 3 * (m - 1) ** 2)
    c4 = 4.0 * (m - 3) / (m ** 3 * (m - 1) ** 2)
    c5 = (8.0 * m - 12.0) / (m ** 5 * (m - 1))
    c6 = 8.0 / (m ** 3 * (m - 1))
    off = 1.0 - torch.eye(m, dtype=K_XX.dtype)
    a, b = (K_XX * off).sum(1), (K_YY * off).sum(1)
    r, c = K_XY.sum(1), K_XY.sum(0)
    A, B, C = a.sum(), b.sum(), c.sum()
    dxx = (c1 * (4 * a[:, None] - 2 * K_XX) - 2 * c2 * A + c6 * (C / m - r[:, None])) * off
    dyy = (c1 * (4 * b[:, None] - 2 * K_YY) - 2 * c2 * B + c6 * (C / m - c[:, None])) * off
    dxy = c3 * (2 * r[:, None] + 2 * c[None, :]) - 2 * c4 * K_XY - 2 * c5 * C + c6 * ((A + B) / m - a[:, None] - b[None, :])
    return dxx, dxy, dyy
