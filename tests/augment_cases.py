"""Shared by tests/golden/make_augment_goldens.py and the augmentation tests: the case table, the stage parameters and the
host restatement of the three per-cloud draws of sug_prepare_batch_aug (counter layout: include/sug_amd.h and
tests/data_pipeline_cases.py, whose Philox restatement this module uses).

New purposes, index 0 each, cloud slot b:
purpose 0x30000000: scale = scale_low + ((word0 >> 8) * 2^-24) * (scale_high - scale_low);
purpose 0x40000000: the three perturbation normals, the Box-Muller of the jitter (words 0, 1 -> two, words 2, 3 -> the third);
purpose 0x50000000: shift_j = (2 * ((word_j >> 8) * 2^-24) - 1) * shift_range, j = 0..2.
"""
import itertools

import numpy as np

import data_pipeline_cases as C

DRAW_SCALE, DRAW_PERTURB, DRAW_SHIFT = 0x30000000, 0x40000000, 0x50000000

# the reference functions' defaults
SCALE_LOW, SCALE_HIGH = 0.8, 1.25
ANGLE_SIGMA, ANGLE_CLIP = 0.06, 0.18
SHIFT_RANGE = 0.1
PLANTED_NORMAL = -3.5                                       # * 0.06 = -0.21: beyond the clip at 0.18

FUNCTIONS = ('shift_point_cloud', 'random_scale_point_cloud', 'rotate_perturbation_point_cloud')
FN_POINTS = C.SHAPES['subset']                              # the function and chain cases: the 96-point unit-scale set


def fn_clouds():
    """The unit-scale 96-point clouds of data_pipeline.npz ('pts_unit_subset'), from the same seed."""
    return C.make_clouds('unit', FN_POINTS, 100 + 10 * C.SETS.index('unit') + FN_POINTS)


def recipe_names():
    """subset_off_rot1, ...: every shape x cloud set x pre-rotation on / off, all five stages on."""
    return ['%s_%s_rot%d' % (s, c, r) for s, c, r in itertools.product(C.SHAPES, C.SETS, (1, 0))]


def recipe_of(name):
    s, c, r = name.split('_')
    return {'shape': s, 'P': C.SHAPES[s], 'set': c, 'pre_rotate': r == 'rot1', 'pts': 'pts_%s_%s' % (c, s)}


def recipe_clouds(kind, shape):
    """The clouds of data_pipeline.npz's 'pts_<kind>_<shape>', from the same seed."""
    P = C.SHAPES[shape]
    return C.make_clouds(kind, P, 100 + 10 * C.SETS.index(kind) + P)


DRAW_KEYS = ('angle', 'noise', 'scales', 'normals', 'shifts')       # per shape: '<key>_<shape>'; 'sel_subset' besides

# DistributedSampler: (dataset length, world size); index lists [shuffle off / on, epoch 0 / 1, rank, num_samples]
SAMPLER_WORLD = 3
SAMPLER_LENGTHS = (10, 9)                                   # 10: one index of padding per epoch; 9: none
SAMPLER_EPOCHS = (0, 1)


class Sized:
    """What a sampler needs of a dataset."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


# ---------------------------------------------------------------------------------------------------------- host draws
def _u24(w):
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def host_scales(seed, counter, B, lo=SCALE_LOW, hi=SCALE_HIGH):
    """[B] fp64"""
    return lo + _u24(C._words(seed, counter, B, DRAW_SCALE, 1)[:, 0, 0]) * (hi - lo)


def host_shifts(seed, counter, B, shift_range=SHIFT_RANGE):
    """[B, 3] fp64"""
    return (2.0 * _u24(C._words(seed, counter, B, DRAW_SHIFT, 1)[:, 0, :3]) - 1.0) * shift_range


def host_perturb_normals(seed, counter, B):
    """[B, 3] fp64: data_pipeline_cases.host_normals' Box-Muller on the one block of the perturbation purpose"""
    w = C._words(seed, counter, B, DRAW_PERTURB, 1)[:, 0].astype(np.uint64)
    u = ((w >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    v = _u24(w)
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = 2.0 * np.pi * v[:, 1], 2.0 * np.pi * v[:, 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1)
