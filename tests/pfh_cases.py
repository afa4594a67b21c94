"""Shared by the PFH tests and tests/golden/make_pfh_goldens.py: a plain numpy fp64 restatement of what
sug_pfh_descriptors and sug_pfh_hist_distance compute (include/sug_amd.h), the synthetic clouds, and the margins that say
how far a cloud keeps every discrete decision from rounding.

Everything works in float64 on the fp32 input values.  Points without a neighbour inside the radius are UNUSED: nbr_cnt 0,
a zero normal, a zero histogram row, no part in distances.
"""
import numpy as np

import splitter_cases

# name -> (N, rad, div, nneighbors): the cases of tests/golden/pfh.npz.  c500_d2 and c500_d5 are one cloud; n9's radius
# covers the cloud, so every point has exactly k = 8 neighbours
CASES = {'c64_d2': (64, 0.45, 2, 8), 'c64_d3': (64, 0.45, 3, 8), 'c130_d2': (130, 0.3, 2, 8), 'c500_d2': (500, 0.2, 2, 8),
         'c500_d5': (500, 0.2, 5, 8), 'n9_d2': (9, 4.0, 2, 8)}
SAME_CLOUD = {'c500_d5': 'c500_d2'}
MARGIN = 1e-9                           # every discrete decision of a golden cloud is at least this far from flipping
GAP = 1e-6                              # and every normal's relative eigen gap at least this
EPS = 2.0 ** -52


def shell(N, g, normal_pc=splitter_cases.normal_pc, fps=splitter_cases.fps):
    """Random directions scaled by U(0.7, 1) * (1, 0.7, 0.5), 4N points, normal_pc, fps to N, snapped to fp32."""
    v = g.standard_normal((4 * N, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    pts = v * g.uniform(0.7, 1.0, (4 * N, 1)) * np.array([1.0, 0.7, 0.5])
    return np.ascontiguousarray(fps(normal_pc(pts), N).astype(np.float32))


def thresholds(div):
    """calc_thresholds: rows alpha, phi, theta."""
    s = np.array([-1 + i * (2. / div) for i in range(1, div)])
    return np.array([s, s, np.array([-np.pi / 2 + i * (np.pi / div) for i in range(1, div)])])


def pair_distances(P):
    dx, dy, dz = (P[:, None, c] - P[None, :, c] for c in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def neighbours(P, rad, k):
    """-> (idx int [N, k] padded with -1, cnt int [N], margin): candidates with distance <= rad, j = i included, ordered by
    (distance, index), the first dropped, the next k kept.  margin: the smallest gap between consecutive kept distances, to
    the first one left out, and between any distance and rad."""
    N = len(P)
    with np.errstate(invalid='ignore'):
        D = pair_distances(P)
        inside = D <= rad
    key = np.where(inside, D, np.inf)
    order = np.argsort(key, axis=1, kind='stable')                 # stable: equal distances stay in index order
    ncand = inside.sum(axis=1)
    cnt = np.clip(ncand - 1, 0, k)
    idx = np.full((N, k), -1, dtype=np.int64)
    take = order[:, 1:k + 1]
    keep = np.arange(take.shape[1])[None, :] < cnt[:, None]
    idx[:, :take.shape[1]][keep] = take[keep]
    srt = np.sort(key, axis=1)[:, :k + 2]                          # the dropped one, the kept ones, the first one left out
    with np.errstate(invalid='ignore'):
        gaps = np.diff(srt, axis=1)                                 # inf - inf past the last candidate
    gaps = gaps[np.isfinite(gaps)]
    margin = min(gaps.min() if gaps.size else np.inf, np.abs(D - rad)[np.isfinite(D)].min())
    return idx, cnt, float(margin)


def normals(P, idx, cnt):
    """-> (normals [N, 3], relative eigen gap (l_mid - l_min) / l_max [N], |normal . p| [N]): the covariance of the neighbours
    about their mean over their count, the eigenvector of its smallest eigenvalue, negated when normal . (-p) < 0.  Unused
    points: zero normal, gap and dot NaN."""
    N = len(P)
    out, gap, dots = np.zeros((N, 3)), np.full(N, np.nan), np.full(N, np.nan)
    for i in range(N):
        if cnt[i] == 0:
            continue
        X = P[idx[i, :cnt[i]]]
        X = X - X.sum(axis=0) / cnt[i]
        w, V = np.linalg.eigh(X.T @ X / cnt[i])                    # ascending eigenvalues
        n = V[:, 0]
        if n @ (-P[i]) < 0:
            n = -n
        out[i] = n
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        dots[i] = abs(n @ P[i])
    return out, gap, dots


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _step(thr, f):
    return np.where(np.isnan(f), len(thr), (f[..., None] >= thr).sum(axis=-1))


def hist_counts(P, nrm, idx, cnt, div):
    """The pair features of p_list = [i] + neighbours binned -> (counts int [N, div^3], margin, largest of |a|, |b|): margin
    is the smallest of |feature - threshold|, |a - b|, |1 - |a||, |1 - |b|| over all pairs whose features are numbers."""
    N, k = idx.shape
    thr = thresholds(div)
    counts = np.zeros((N, div ** 3), dtype=np.int64)
    L = np.concatenate((np.arange(N)[:, None], idx), axis=1)
    margin, ab_max = np.inf, 0.0
    rows = np.arange(N)
    with np.errstate(all='ignore'):
        for zi in range(k + 1):
            for pi in range(zi + 1, k + 1):
                valid = pi < cnt + 1
                if not valid.any():
                    continue
                z, p = L[valid, zi], L[valid, pi]
                Pz, Pp, nz, npp = P[z], P[p], nrm[z], nrm[p]
                a, b = _dot(npp, Pz - Pp), _dot(nz, Pp - Pz)
                p_src = ((np.abs(a) <= 1) & (np.abs(b) <= 1) & (a >= b))[:, None]
                ps, pt = np.where(p_src, Pp, Pz), np.where(p_src, Pz, Pp)
                u, nt = np.where(p_src, npp, nz), np.where(p_src, nz, npp)
                d = pt - ps
                d = d / np.sqrt(_dot(d, d))[:, None]
                v = np.cross(d, u)
                w = np.cross(u, v)
                f = (_dot(v, nt), _dot(u, d), np.arctan(_dot(w, nt) / _dot(u, nt)))
                b_idx = _step(thr[0], f[0]) + div * _step(thr[1], f[1]) + div * div * _step(thr[2], f[2])
                np.add.at(counts, (rows[valid], b_idx), 1)
                ok = ~np.isnan(f[0] + f[1] + f[2])
                parts = [np.abs(f[c][ok, None] - thr[c]).ravel() for c in range(3)]
                parts += [np.abs(a - b)[ok], np.abs(1 - np.abs(a))[ok], np.abs(1 - np.abs(b))[ok]]
                ab_max = max([ab_max] + [float(np.abs(x[ok]).max()) for x in (a, b) if ok.any()])
                m = min((x.min() for x in parts if x.size), default=np.inf)
                margin = min(margin, m)
    return counts, float(margin), ab_max


def npairs(k):
    return (k + 1) * k // 2                                         # comb(k + 1, 2)


def descriptors(pts, rad, k, div):
    """The whole of sug_pfh_descriptors for one cloud -> dict(idx, cnt, normals, gap, counts, hist, margin, used_cnt)."""
    P = np.asarray(pts, dtype=np.float64)
    idx, cnt, m_n = neighbours(P, rad, k)
    nrm, gap, dots = normals(P, idx, cnt)
    counts, m_h, ab_max = hist_counts(P, nrm, idx, cnt, div)
    return {'ab_max': ab_max, 'idx': idx, 'cnt': cnt, 'normals': nrm, 'gap': gap, 'dots': dots, 'counts': counts,
            'hist': counts / float(npairs(k)), 'margin': min(m_n, m_h), 'used_cnt': int((cnt > 0).sum())}


def hist_distance(hS, usedS, hT, usedT):
    """pfh_hist_distance on the used rows: the median over the rows of S of the distance to the nearest row of T."""
    a, b = np.asarray(hS, dtype=np.float64)[np.asarray(usedS, bool)], np.asarray(hT, dtype=np.float64)[np.asarray(usedT, bool)]
    if len(a) == 0 or len(b) == 0:
        return float('nan')
    e = a[:, None, :] - b[None, :, :]
    return float(np.median(np.sqrt((e * e).sum(axis=-1)).min(axis=1)))


def normal_bound(gap):
    """Per point: 64 * 2^-52 / gap."""
    return 64 * EPS / gap


def distance_bound(D):
    """Relative: (D + 2) * 2^-52."""
    return (D + 2) * EPS
