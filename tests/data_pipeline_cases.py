"""Shared by tests/golden/make_data_pipeline_goldens.py and the data-pipeline tests: the case table, the seeded inputs,
and the host restatement of the kernel's generator (Philox4x32-10 and the counter layout of include/sug_amd.h).

Counter layout (restated from the header): key = (seed & 0xffffffff, seed >> 32); counter words
    (c & 0xffffffff, c >> 32, cloud slot b, purpose | index),   c = the 64-bit batch counter,
purpose 0x00000000, index 0: the angle, (word0 >> 8) * 2^-24 * 2 pi;
purpose 0x10000000, index q: words 0..3 are the sort keys of points 4q .. 4q+3; kept = the first N of the stable argsort;
purpose 0x20000000, index n: the normals of output row n: r(w0) cos(2 pi v(w1)), r(w0) sin(2 pi v(w1)), r(w2) cos(2 pi v(w3))
    with u(w) = ((w >> 8) + 1) * 2^-24, v(w) = (w >> 8) * 2^-24, r(w) = sqrt(-2 ln u(w)).
"""
import itertools

import numpy as np

DRAW_ANGLE, DRAW_SUBSET, DRAW_NOISE = 0x00000000, 0x10000000, 0x20000000

# ---------------------------------------------------------------------------------------------------------------- cases
N_OUT = 64
SHAPES = {'subset': 96, 'pad': 48, 'same': 64}              # name -> P  (N = 64)
SETS = ('off', 'unit')                                      # off-centre and badly scaled (6 channels) | unit scale (3 channels)
CLOUDS_PER_SET = 2
SIGMA, CLIP = 0.01, 0.05
PLANTED = (6.0, -7.5, 5.2, -5.01)                           # standard-normal draws beyond +-5 sigma: the clip at 0.05 acts


def case_names():
    """subset_off_aug1_rot0, ...: every shape x cloud set x aug on / off x pre-rotation on / off."""
    return ['%s_%s_aug%d_rot%d' % (s, c, a, r) for s, c, a, r in itertools.product(SHAPES, SETS, (1, 0), (1, 0))]


def case_of(name):
    s, c, a, r = name.split('_')
    return {'shape': s, 'P': SHAPES[s], 'set': c, 'aug': a == 'aug1', 'pre_rotate': r == 'rot1', 'pts': 'pts_%s_%s' % (c, s),
            'noise': 'noise_%s' % s, 'angle': 'angle_%s' % s, 'sel': 'sel_%s' % s}


def make_clouds(kind, P, seed):
    """[CLOUDS_PER_SET, P, C] fp32.  'off': anisotropic extent up to 3, centroid offset up to 2, three extra channels holding
    large values that must not be read; 'unit': within the unit cube."""
    rng = np.random.RandomState(seed)
    if kind == 'unit':
        return rng.uniform(-0.5, 0.5, size=(CLOUDS_PER_SET, P, 3)).astype(np.float32)
    xyz = rng.uniform(-1.5, 1.5, size=(CLOUDS_PER_SET, P, 3)) * np.array([1.0, 0.3, 0.05])
    xyz = xyz + rng.uniform(-2.0, 2.0, size=(CLOUDS_PER_SET, 1, 3))
    extra = rng.uniform(100.0, 200.0, size=(CLOUDS_PER_SET, P, 3))
    return np.concatenate([xyz, extra], axis=2).astype(np.float32)


# function cases of data_utils: name -> (function, cloud key, extra arguments)
ROTATE_SHAPE_CASES = (('x', -np.pi / 2), ('y', 0.3), ('z', 1.1))

# cls_wights / Sampler
CLASS_COUNTS = (30, 5, 12, 7, 50, 3, 9, 21, 4, 16)
WEIGHTINGS = (('number_inverse', None), ('exp_inverse', None), ('DLSA', None), ('DLSA', 0.7), ('DLSA', 'kl'), ('uniform', None))
SAMPLER_ARGS = (4, 8)                                       # class_per_batch, batch_size
SAMPLER_SEED, SAMPLER_BATCHES = 0, 10


def labels_list():
    """157 labels with CLASS_COUNTS members per class, interleaved by a fixed permutation."""
    lab = np.concatenate([np.full(n, k) for k, n in enumerate(CLASS_COUNTS)])
    return lab[np.random.RandomState(5).permutation(lab.size)]


# ---------------------------------------------------------------------------------------------------------------- Philox
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4] and key (k0, k1) of 32-bit words -> [..., 4] uint32 (Salmon et al., SC'11)."""
    c = np.asarray(ctr, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                          # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _words(seed, counter, B, purpose, count):
    """[B, count, 4] words of the Philox blocks (counter, slot b, purpose | i), i < count."""
    ctr = np.zeros((B, count, 4), dtype=np.uint64)
    ctr[..., 0] = counter & 0xFFFFFFFF
    ctr[..., 1] = (counter >> 32) & 0xFFFFFFFF
    ctr[..., 2] = np.arange(B)[:, None]
    ctr[..., 3] = purpose | np.arange(count)[None, :]
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def host_angles(seed, counter, B):
    """[B] fp64"""
    w = _words(seed, counter, B, DRAW_ANGLE, 1)[:, 0, 0]
    return (w >> 8).astype(np.float64) * 2.0 ** -24 * 2.0 * np.pi


def host_subset(seed, counter, B, P, N):
    """[B, N]: the first N points in ascending (word, point) order"""
    P2 = 4
    while P2 < P:
        P2 *= 2
    keys = _words(seed, counter, B, DRAW_SUBSET, P2 // 4).reshape(B, P2)[:, :P]
    return np.argsort(keys, axis=1, kind='stable')[:, :N].astype(np.int32)


def host_normals(seed, counter, B, N):
    """[B, N, 3] fp64 Box-Muller normals of the output rows"""
    w = _words(seed, counter, B, DRAW_NOISE, N).astype(np.uint64)
    u = (((w >> np.uint64(8)) + np.uint64(1)).astype(np.float64)) * 2.0 ** -24
    v = (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    t0, t1 = 2.0 * np.pi * v[..., 1], 2.0 * np.pi * v[..., 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1)


PHILOX_KAT = (                                               # counter, key -> output (the Random123 known-answer vectors)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
