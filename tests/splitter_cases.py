"""Shared by the sub-domain splitter tests and tests/golden/make_splitter_goldens.py: the numpy fp64 restatement of what
sug_amd.dataset_splitter computes, the synthetic clouds, and the builder of the fixture tests/golden/splitter.npz.

The restatement follows include/sug_amd.h (sug_icp_fitness) and the reference's dataset_splitter.py / data/data_utils.py
line by line in float64 on the fp32 input values: normal_pc, fps (from point 0), icp (np.linalg.svd), the split rule and
entropy_clustering.  open3d itself is not available to these tests; the assumptions under which this restates its
registration_icp are written next to the declaration in the header.
"""
import numpy as np

R_CORR = 0.15
N_CLASS, N_PTS = 96, 64                 # the class of clouds: 3 families x 32
ANCHOR = 30                             # source of the 96 pairs (position in `clouds`)
ODD_NS, ODD_NT, N_ODD = 61, 77, 8       # odd sizes, no multiple of the wave
N_BIG, BIG = 2, 500                     # the splitter's own size: two source points per lane
ITER_SETTINGS = (0, 1, 30)
FAMILIES = ('sphere', 'box', 'cylinder')
ENT_ROWS, ENT_CLASSES = 257, 10
PROCESS_M, PROCESS_P, PROCESS_N = 4, 128, 32


# ------------------------------------------------------------------------------------------------------- restatement
def normal_pc(pc):
    """data/data_utils.py:5-15."""
    pc = pc - pc.mean(axis=0)
    return pc / np.max(np.sqrt(np.sum(abs(pc ** 2), axis=-1)))


def fps_index(points, n_samples, margins=None):
    """data/data_utils.py:185-229, returning the indices: start at point 0, running minimum of the squared distance to the
    chosen points, arg-max over the remaining points in ascending order (ties -> lowest index).  margins: a list that
    receives, per step, the relative gap between the largest and the second largest candidate distance."""
    points = np.asarray(points)
    left = np.arange(len(points))
    inds = np.zeros(n_samples, dtype='int')
    dists = np.ones_like(left) * float('inf')
    left = np.delete(left, 0)
    for i in range(1, n_samples):
        last = inds[i - 1]
        d = ((points[last] - points[left]) ** 2).sum(-1)
        dists[left] = np.minimum(d, dists[left])
        sel = np.argmax(dists[left])
        if margins is not None and len(left) > 1:
            top = np.sort(dists[left])[-2:]
            margins.append((top[1] - top[0]) / top[1])
        inds[i] = left[sel]
        left = np.delete(left, sel)
    return inds


def fps(points, n_samples):
    return np.asarray(points)[fps_index(points, n_samples)]


def evaluate(p, q, r2):
    """-> (mask of the correspondences, nearest target per source point, its d2)."""
    dx, dy, dz = (p[:, None, c] - q[None, :, c] for c in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    j = d2.argmin(axis=1)                               # first occurrence: the lowest index wins a tie
    best = d2[np.arange(len(p)), j]
    return best < r2, j, best


def _result(mask, best):
    n = int(mask.sum())
    return n, (float(np.sqrt(best[mask].sum() / n)) if n else 0.0)


def umeyama_update(P, Q):
    """Eigen::umeyama without scaling on correspondences p_i -> q_i: (R, t, singular values of Sigma)."""
    pm, qm = P.mean(axis=0), Q.mean(axis=0)
    sigma = (Q - qm).T @ (P - pm) / len(P)
    U, s, Vt = np.linalg.svd(sigma)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    return R, qm - R @ pm, s


def icp(src, tgt, max_corr_dist=R_CORR, max_iteration=30, rel_fitness=1e-6, rel_rmse=1e-6, trace=None):
    """registration_icp as include/sug_amd.h restates it -> (count, rmse, iters, transform [4, 4]).  trace: a dict that
    receives 'r2_margin' (the smallest |d2 - r*r| / (r*r) over every nearest neighbour of every evaluation) and 'sv' (the
    singular values of the first update's Sigma)."""
    p, q = np.asarray(src, dtype=np.float64).copy(), np.asarray(tgt, dtype=np.float64)
    r2 = max_corr_dist * max_corr_dist
    T = np.eye(4)

    def note(best):
        if trace is not None:
            trace['r2_margin'] = min(trace.get('r2_margin', np.inf), float(np.abs(best - r2).min() / r2))

    mask, j, best = evaluate(p, q, r2)
    note(best)
    count, rmse = _result(mask, best)
    iters = 0
    for _ in range(max_iteration):
        if count == 0:
            break
        R, t, s = umeyama_update(p[mask], q[j[mask]])
        if trace is not None and iters == 0:
            trace['sv'] = s
        p = p @ R.T + t
        U = np.eye(4)
        U[:3, :3], U[:3, 3] = R, t
        T = U @ T
        iters += 1
        prev = (count / len(p), rmse)
        mask, j, best = evaluate(p, q, r2)
        note(best)
        count, rmse = _result(mask, best)
        if abs(prev[0] - count / len(p)) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
            break
    return count, rmse, iters, T


def icp_batch(srcs, tgts, max_iteration, traces=None):
    """srcs [Ns, 3] (one source) or [B, Ns, 3] -> dict of arrays count / rmse / iters / transform."""
    B = len(tgts)
    out = {'count': np.zeros(B, np.int32), 'rmse': np.zeros(B), 'iters': np.zeros(B, np.int32), 'transform': np.zeros((B, 4, 4))}
    for b in range(B):
        tr = {} if traces is not None else None
        c, r, i, T = icp(srcs if np.ndim(srcs) == 2 else srcs[b], tgts[b], max_iteration=max_iteration, trace=tr)
        out['count'][b], out['rmse'][b], out['iters'][b], out['transform'][b] = c, r, i, T
        if traces is not None:
            traces.append(tr)
    return out


def icp_distance(src, tgt):
    return 1 - icp(src, tgt)[0] / len(src)


def split_rule(distances, use_hist=False):
    """dataset_splitter.py:62-69 -> (labels, accepted)."""
    d = np.asarray(distances, dtype=np.float64)
    n = len(d)
    pos = np.where(d < (np.histogram(d, bins=2)[1][1] if use_hist else np.mean(d)))
    labels = np.ones(n)
    labels[pos] = 0
    return labels.astype(np.int64), bool(np.abs(pos[0].shape[0] - 0.5 * n) < 0.4 * n)


def split_class(raw, anchors, use_hist=False, pt_num=N_PTS):
    """dataset_splitter.py:43-79 for one class with the anchor draws given -> (order, labels, distances, anchor, tries)."""
    order = np.argsort(raw[:, :, 0].min(axis=1), kind='stable')          # sorted(raw, key=x_min)
    processed = [fps(normal_pc(raw[i].astype(np.float64)), pt_num).astype(np.float32) for i in order]
    for tries, a in enumerate(anchors[:5], 1):
        d = np.array([icp_distance(processed[a], c) for c in processed])
        labels, ok = split_rule(d, use_hist)
        if ok:
            break
    return order, labels, d, a, tries


def entropy_clustering(probs, cluster_num=4):
    """dataset_splitter.py:191-214 in float64 -> (labels, entropies)."""
    probs = np.asarray(probs, dtype=np.float64)
    u = -(probs * np.log(probs + 1e-30)).sum(1)
    labels = np.ones(len(u))
    edges = np.histogram(u, bins=cluster_num)[1]
    for i in range(cluster_num):
        labels[np.where((u >= edges[i]) & (u < edges[i + 1]))] = i
    return labels.astype(np.int64), u


def edge_margin(u, cluster_num):
    """Smallest distance of an entropy to an edge it does not define (the smallest and the largest entropy ARE the outer
    edges; every other row must keep clear of all of them)."""
    edges = np.histogram(u, bins=cluster_num)[1]
    inner = np.delete(u, [u.argmin(), u.argmax()])
    return float(np.abs(inner[:, None] - edges[None, :]).min())


# ------------------------------------------------------------------------------------------------------------ clouds
def _rotation(g, max_angle):
    a = g.uniform(-max_angle, max_angle, 3)
    cx, cy, cz, sx, sy, sz = *np.cos(a), *np.sin(a)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_cloud(family, n, g, thin=False):
    """One cloud of a family with 0.01 noise, slightly rotated, through normal_pc, as fp32 [n, 3]."""
    if family == 'sphere':                                   # scaled sphere
        v = g.normal(size=(n, 3))
        x = v / np.linalg.norm(v, axis=1, keepdims=True) * g.uniform(0.75, 1.0, 3)
    elif family == 'box':                                    # box shell
        x = g.uniform(-1, 1, size=(n, 3))
        face = g.integers(0, 3, n)
        x[np.arange(n), face] = np.sign(g.uniform(-1, 1, n))
        x = x * g.uniform(0.5, 0.65, 3)
    else:                                                    # cylinder: lateral surface and the two caps
        radius, height = (0.03, 2.0) if thin else (g.uniform(0.45, 0.6), g.uniform(1.0, 1.3))
        phi, cap = g.uniform(0, 2 * np.pi, n), g.uniform(0, 1, n) < 0.25
        rr = np.where(cap, radius * np.sqrt(g.uniform(0, 1, n)), radius)
        z = np.where(cap, np.sign(g.uniform(-1, 1, n)) * height / 2, g.uniform(-height / 2, height / 2, n))
        x = np.stack((rr * np.cos(phi), rr * np.sin(phi), z), axis=1)
    x = x @ _rotation(g, 0.2).T + 0.01 * g.normal(size=(n, 3))
    return normal_pc(x).astype(np.float32)


def make_class(seed, m=N_CLASS, n=N_PTS):
    """m clouds, the three families in turn."""
    g = np.random.default_rng(seed)
    return np.stack([make_cloud(FAMILIES[i % 3], n, g) for i in range(m)])


def make_probs(seed, rows=ENT_ROWS, classes=ENT_CLASSES):
    g = np.random.default_rng(seed)
    z = g.normal(size=(rows, classes)) * g.uniform(0.2, 4.0, size=(rows, 1))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- fixture
SEEDS = {'clouds': 21, 'odd': 12, 'big': 13, 'probs': 14, 'process': 15, 'thin': 16}
SPLIT_ANCHORS = (30, 27, 33, 36, 40)     # positions in the sorted order: the mean cut accepts the first, the histogram
                                         # cut (only the anchor itself lies below the middle edge) refuses all five
REDRAW_COPIES = (4, 14)                  # the redraw class: `thin` and ten copies each of a box and a cylinder


def inputs():
    """The fixture's input arrays, from the seeds."""
    out = {'clouds': make_class(SEEDS['clouds'])}
    # a cylinder too thin to register with anything: as an anchor every other cloud is about equally far (d close to 1),
    # so only the anchor itself falls below the mean and the balance test fails
    out['thin'] = make_cloud('cylinder', N_PTS, np.random.default_rng(SEEDS['thin']), thin=True)
    g = np.random.default_rng(SEEDS['odd'])
    out['odd_src'] = np.stack([make_cloud(FAMILIES[i % 3], ODD_NS, g) for i in range(N_ODD)])
    out['odd_tgt'] = np.stack([make_cloud(FAMILIES[(i + i // 4) % 3], ODD_NT, g) for i in range(N_ODD)])
    g = np.random.default_rng(SEEDS['big'])
    out['big_src'] = np.stack([make_cloud(FAMILIES[i], BIG, g) for i in range(N_BIG)])
    out['big_tgt'] = np.stack([make_cloud(FAMILIES[i], BIG, g) for i in range(N_BIG)])
    out['probs'] = make_probs(SEEDS['probs'])
    g = np.random.default_rng(SEEDS['process'])
    # raw clouds as a dataset holds them: off-centre, not unit scale
    out['process_raw'] = np.stack([make_cloud(FAMILIES[i % 3], PROCESS_P, g) * g.uniform(0.5, 3) + g.uniform(-1, 1, 3)
                                   for i in range(PROCESS_M)]).astype(np.float32)
    return out


PAIR_SETS = {'cls': ('clouds', None), 'odd': ('odd_tgt', 'odd_src'), 'big': ('big_tgt', 'big_src')}


def pairs_of(fx, name):
    """(source, targets) of a pair set: the class registers its ANCHOR cloud against every cloud."""
    tgt, src = PAIR_SETS[name]
    return (fx[src] if src else fx['clouds'][ANCHOR]), fx[tgt]


def redraw_class(fx):
    """-> (raw clouds [21, 64, 3] of the redraw class, its two anchors as positions in the sorted order: `thin`, whose try
    fails the balance test, then a copy of the box, whose try passes: its ten copies against the rest)."""
    raw = np.stack([fx['thin']] + [fx['clouds'][i] for i in REDRAW_COPIES for _ in range(10)])
    order = np.argsort(raw[:, :, 0].min(axis=1), kind='stable')
    return raw, (int(np.flatnonzero(order == 0)[0]), int(np.flatnonzero(order == 1)[0]))


def results(fx, traces=None):
    """Everything the fixture records about its inputs `fx`, from the restatement."""
    out = {}
    for name in PAIR_SETS:
        src, tgt = pairs_of(fx, name)
        for it in ITER_SETTINGS:
            tr = [] if (traces is not None and it == 30) else None
            r = icp_batch(src, tgt, it, tr)
            for k, v in r.items():
                out['%s_it%d_%s' % (name, it, k)] = v
            if tr is not None:
                traces[name] = tr
    for use_hist in (False, True):
        tag = 'hist' if use_hist else 'mean'
        order, labels, d, a, tries = split_class(fx['clouds'], SPLIT_ANCHORS, use_hist)
        out['split_%s_order' % tag], out['split_%s_labels' % tag], out['split_%s_dist' % tag] = order, labels, d
        out['split_%s_tries' % tag] = np.int64(tries)
    raw, redraw = redraw_class(fx)
    order, labels, d, a, tries = split_class(raw, redraw)
    out['redraw_anchors'], out['redraw_labels'], out['redraw_tries'] = np.array(redraw), labels, np.int64(tries)
    for k in (2, 4):
        out['ent_labels_%d' % k], out['ent_u'] = entropy_clustering(fx['probs'], k)
    margins = []
    normed = [normal_pc(c.astype(np.float64)) for c in fx['process_raw']]
    out['process_idx'] = np.stack([fps_index(c, PROCESS_N, margins) for c in normed]).astype(np.int32)
    out['process_pts'] = np.stack([c[i] for c, i in zip(normed, out['process_idx'])])
    out['process_margin'] = np.float64(min(margins))
    return out
