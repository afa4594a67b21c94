"""Shared by the part-segmentation loader tests (test_seg_loader_host.py, test_gpu_seg_loader.py): the case table, the seeded
inputs, the host restatement of the fill draw of sug_prepare_seg_batch and the fp64 recipe of its contract
(include/sug_amd.h).  The old draws are data_pipeline_cases' and augment_cases' restatements.

New purpose (counter layout: data_pipeline_cases): 0x60000000, index i: word j of the block is the draw of fill row
n = L + 4 i + j of a cloud of L <= N points; its source point is (uint64(word) * L) >> 32.
"""
import numpy as np

import augment_cases as A
import data_pipeline_cases as C

DRAW_FILL = 0x60000000
SEED = 0x1234567887654321

# name -> P, N, the lengths of the resident clouds (M = their number; a batch takes them all in order)
CASES = {
    'small': dict(P=96, N=64, lengths=(96, 70, 64, 41, 5)),     # subset, subset, identity, a fill of 23 rows (a partial Philox
                                                                # block), a fill of 59 rows; 256 threads
    'mid': dict(P=600, N=256, lengths=(600, 256, 130)),         # 512 threads
    'big': dict(P=4096, N=2048, lengths=(4096, 2500)),          # the smallest shape with > 64 KB of LDS and 1024 threads
}

# fp32 roundings that reach one output coordinate, per stage: the table derived in tests/test_gpu_augment.py's docstring
# (coordinates below 2 in magnitude, -ffp-contract=off: a product and a sum are two roundings), restated.  One rounding of a
# value below 2 moves it by at most 2^-24.
ROUNDINGS = {'normalize': 6, 'pre': 8, 'rotate_z': 7, 'jitter': 2, 'scale': 1, 'perturb': 9, 'shift': 1}
NORMAL_STAGES = ('pre', 'rotate_z', 'perturb')                  # what a direction channel goes through
FIVE = ('rotate_z', 'jitter', 'scale', 'perturb', 'shift')
PARAMS = dict(scale_low=A.SCALE_LOW, scale_high=A.SCALE_HIGH, shift_range=A.SHIFT_RANGE, angle_sigma=A.ANGLE_SIGMA,
              angle_clip=A.ANGLE_CLIP)
COORD_BOUND = 2.0


def bound(stages):
    return sum(ROUNDINGS[s] for s in stages) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_case(name, extra_channels=3):
    """-> dict: pts [M, P, 3] fp32 ('unit' clouds: within the unit cube), extra [M, P, E] fp32 (channels 0..2 unit vectors, the
    rest uniform in [-3, 3]), point_label [M, P] uint8 planted as a function of (cloud, point), category [M] int64,
    lengths [M] int32, and P, N, M."""
    c = CASES[name]
    P, N, lengths = c['P'], c['N'], np.array(c['lengths'], dtype=np.int32)
    M = len(lengths)
    pts = np.concatenate([C.make_clouds('unit', P, 700 + 10 * i + P) for i in range((M + 1) // 2)])[:M]
    assert pts.shape == (M, P, 3) and np.abs(pts).max() <= 0.5
    r = np.random.RandomState(P + extra_channels)
    extra = None
    if extra_channels:
        v = r.randn(M, P, 3)
        parts = [v / np.linalg.norm(v, axis=2, keepdims=True)]
        if extra_channels > 3:
            parts.append(r.uniform(-3.0, 3.0, size=(M, P, extra_channels - 3)))
        extra = np.concatenate(parts, axis=2)[:, :, :extra_channels].astype(np.float32)
    m, p = np.arange(M)[:, None], np.arange(P)[None, :]
    label = ((11 * m + 7 * p + p // 64) % 61).astype(np.uint8)
    category = ((3 * np.arange(M) + 1) % 16).astype(np.int64)
    return dict(pts=pts, extra=extra, point_label=label, category=category, lengths=lengths, P=P, N=N, M=M)


# ---------------------------------------------------------------------------------------------------------------- draws
def fill_sources(words, L):
    """(uint64(word) * L) >> 32 for each 32-bit word: uniform over [0, L)."""
    return ((np.asarray(words, dtype=np.uint64) * np.uint64(L)) >> np.uint64(32)).astype(np.int32)


def host_fill(seed, counter, b, L, N):
    """[N - L] int32: the source points of rows L .. N-1 of the cloud in batch slot b (L <= N)."""
    n = N - L
    if n <= 0:
        return np.zeros(0, dtype=np.int32)
    words = C._words(seed, counter, b + 1, DRAW_FILL, (n + 3) // 4)[b].reshape(-1)[:n]
    return fill_sources(words, L)


def host_sources(seed, counter, b, L, N):
    """[N] int32: the source point of every output row without SUG_PREP_SHUFFLE."""
    if L > N:
        return C.host_subset(seed, counter, b + 1, L, N)[b]
    return np.concatenate([np.arange(L, dtype=np.int32), host_fill(seed, counter, b, L, N)])


# ---------------------------------------------------------------------------------------------------------------- fp64 recipe
def perturb_matrix(normals, angle_sigma=A.ANGLE_SIGMA, angle_clip=A.ANGLE_CLIP):
    """R = Rz (Ry Rx) of rotate_perturbation_point_cloud from three standard normals, in fp64."""
    ax, ay, az = np.clip(angle_sigma * np.asarray(normals, dtype=np.float64), -angle_clip, angle_clip)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ (Ry @ Rx)


def recipe(pts, extra, L, src, stages, *, pre=None, angle=0.0, noise=None, scale=1.0, normals=None, shift=None, turn=False,
           sigma=C.SIGMA, clip=C.CLIP):
    """One cloud in fp64: pts [P, 3], extra [P, E] or None, its length L, src [N] (the source point of every row), `stages` a
    collection of ROUNDINGS' names, the draws as the kernel reports them (noise [N, 3]: the normals of the output rows).
    -> [3 + E, N] fp64.  turn: channels 0..2 of extra go through the three rotations (SUG_PREP_NORMALS)."""
    x = np.asarray(pts, dtype=np.float64)[:L]
    if 'normalize' in stages:
        x = x - x.mean(axis=0)
        x = x / np.sqrt((x * x).sum(axis=1).max())
    x = x[src]
    rots = []
    if pre is not None:
        rots.append(np.asarray(pre, dtype=np.float64).reshape(3, 3))
    if 'rotate_z' in stages:
        c, s = np.cos(float(angle)), np.sin(float(angle))
        rots.append(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]))
    if rots:
        for R in rots:
            x = x @ R
    if 'jitter' in stages:
        x = x + np.clip(sigma * np.asarray(noise, dtype=np.float64), -clip, clip)
    if 'scale' in stages:
        x = x * float(scale)
    if 'perturb' in stages:
        Rp = perturb_matrix(normals)
        x = x @ Rp
        rots.append(Rp)
    if 'shift' in stages:
        x = x + np.asarray(shift, dtype=np.float64)
    assert np.abs(x).max() < COORD_BOUND, 'the tolerance assumes coordinates below 2'
    out = [x]
    if extra is not None:
        e = np.asarray(extra, dtype=np.float64)[src]
        if turn:
            d = e[:, :3]
            for R in rots:
                d = d @ R
            e = np.concatenate([d, e[:, 3:]], axis=1)
        out.append(e)
    return np.concatenate(out, axis=1).T
