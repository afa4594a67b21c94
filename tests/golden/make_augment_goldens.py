#!/usr/bin/env python3
"""Generate tests/golden/augment.npz by RUNNING THE REFERENCE's data/data_utils.py (shift_point_cloud,
random_scale_point_cloud, rotate_perturbation_point_cloud and the rest of pc_augment's lines) and its DistributedSampler
(data/dataloader.py) (build container only, CPU).

Usage (from the repo root, a few seconds):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_augment_goldens.py

Uses make_goldens.py's set-up and make_data_pipeline_goldens.py's recorded draws; cases and inputs come from
tests/augment_cases.py, which the tests share.  On top of the angle / jitter / shuffle draws recorded there:
  * uniform(lo, hi, size) returns fp32-representable values (size 1: the scale, size 3: the shift);
  * randn(3) -- told apart from the jitter's randn(*pc.shape) by its shape -- returns fp32-representable normals, the second
    of the first call planted beyond the clip of the perturbation angles.
shift_point_cloud / random_scale_point_cloud work in place: they get copies.  Per case the fixture holds the reference on
fp32 input cast to fp32 (`ref32`), the same functions on float64 input (`ref64`) and dev_ref = max |ref32 - ref64|."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as MG                          # noqa: E402  (stubs, reference on sys.path)
import make_data_pipeline_goldens as DP            # noqa: E402  (the recorded-draw wrappers)

import data.data_utils as r_du                     # noqa: E402  (reference)
import data.dataloader as r_dl                     # noqa: E402

import augment_cases as A                          # noqa: E402
import data_pipeline_cases as C                    # noqa: E402


class Draws(DP.Draws):
    """DP.Draws plus uniform(lo, hi, size) and randn(3)."""

    def reset(self):
        super().reset()
        self.rng_a = np.random.RandomState(self.seed + 3)
        self.scales, self.normals, self.shifts = [], [], []

    def uniform(self, low=None, high=None, size=None):
        if low is None:
            return super().uniform()
        v = self.rng_a.uniform(low, high, size).astype(np.float32)
        {1: self.scales, 3: self.shifts}[v.size].append(v)
        return v.astype(np.float64)

    def randn(self, *shape):
        if shape != (3,):
            return super().randn(*shape)
        n = self.rng_a.standard_normal(3).astype(np.float32)
        if not self.normals:
            n[1] = A.PLANTED_NORMAL
        self.normals.append(n)
        return n.astype(np.float64)

    def recorded(self):
        return {'angle': np.array(self.angles, dtype=np.float32).reshape(-1), 'noise': np.array(self.noise, dtype=np.float32),
                'scales': np.array(self.scales, dtype=np.float32).reshape(-1), 'normals': np.array(self.normals, dtype=np.float32),
                'shifts': np.array(self.shifts, dtype=np.float32), 'perms': np.array(self.perms)}


def chain(x):
    """pc_augment with every line switched on, in its line order"""
    x = r_du.rotation_point_cloud(x)
    x = r_du.jitter_point_cloud(x)
    x = r_du.random_scale_point_cloud(np.array(x))
    x = r_du.rotate_perturbation_point_cloud(x)
    return r_du.shift_point_cloud(np.array(x))


def recipe(raw, dtype, pre_rotate, num_points):
    """UnifiedPointDG.__getitem__ (data/dataloader.py:302-327) with chain() in pc_augment's place"""
    x = r_du.normal_pc(raw[:, :3].astype(dtype))
    if pre_rotate:
        a = -np.pi / 2
        if dtype == np.float32:
            x = r_du.rotate_shape(x, 'x', a)
        else:           # rotate_shape casts its result to float32; the fp64 value is its product without the cast
            x = x.dot(np.asarray([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]))
    x = chain(x)
    if x.shape[0] < num_points:
        x = np.concatenate((x, np.zeros((num_points - x.shape[0], 3), dtype=float)), axis=0)
    elif x.shape[0] > num_points:
        point_idx = np.arange(0, x.shape[0])
        np.random.shuffle(point_idx)
        x = x[point_idx[:num_points]]
    return x.transpose()


def both(out, key, fn, clouds, seed):
    """fn on every cloud as fp32 (result cast to fp32) and as fp64, with the same recorded draws -> the draws"""
    d = Draws(seed)
    with d:
        r32 = np.stack([np.asarray(fn(np.array(x, dtype=np.float32))).astype(np.float32) for x in clouds])
    rec = d.recorded()
    d.reset()
    with d:
        r64 = np.stack([np.asarray(fn(np.array(x, dtype=np.float64)), dtype=np.float64) for x in clouds])
    again = d.recorded()
    assert all(np.array_equal(rec[k], again[k]) for k in rec), key
    dev = float(np.abs(r32.astype(np.float64) - r64).max())
    assert dev < 1e-5, '%s: the fp64 run is not the fp32 run (dev %g)' % (key, dev)
    out[key + '_ref32'], out[key + '_ref64'], out[key + '_dev_ref'] = r32, r64, np.float64(dev)
    print('%-40s dev_ref %.2e' % (key, dev))
    return rec


def function_cases(out):
    pts = A.fn_clouds()
    out['pts_unit'] = pts
    M = len(pts)
    rec = both(out, 'fn_shift_point_cloud', r_du.shift_point_cloud, pts, 3000)
    out['fn_shifts'] = rec['shifts']
    rec = both(out, 'fn_random_scale_point_cloud', r_du.random_scale_point_cloud, pts, 3001)
    out['fn_scales'] = rec['scales']
    rec = both(out, 'fn_rotate_perturbation_point_cloud', r_du.rotate_perturbation_point_cloud, pts, 3002)
    out['fn_normals'] = rec['normals']
    assert out['fn_shifts'].shape == (M, 3) and out['fn_scales'].shape == (M,) and out['fn_normals'].shape == (M, 3)
    assert abs(A.ANGLE_SIGMA * out['fn_normals'][0, 1]) > A.ANGLE_CLIP             # the clip acts
    rec = both(out, 'chain', chain, pts, 3003)
    for k in A.DRAW_KEYS:
        out['chain_' + k] = rec[k]
    assert rec['noise'].shape == (M, A.FN_POINTS, 3) and (np.abs(rec['noise']) > 5).sum() >= len(C.PLANTED)


def recipe_cases(out):
    for name in A.recipe_names():
        c = A.recipe_of(name)
        pts = A.recipe_clouds(c['set'], c['shape'])
        out[c['pts']] = pts
        rec = both(out, name, lambda x: recipe(x, x.dtype.type, c['pre_rotate'], C.N_OUT), pts, 4000 + c['P'])
        assert out[name + '_ref32'].shape == (len(pts), 3, C.N_OUT)
        for k in A.DRAW_KEYS:                               # the same draws for every case of a shape
            key = '%s_%s' % (k, c['shape'])
            assert key not in out or np.array_equal(out[key], rec[k]), key
            out[key] = rec[k]
        if c['P'] > C.N_OUT:
            sel = rec['perms'][:, :C.N_OUT].astype(np.int32)
            assert 'sel_' + c['shape'] not in out or np.array_equal(out['sel_' + c['shape']], sel)
            out['sel_' + c['shape']] = sel
        else:
            assert rec['perms'].size == 0
        if c['P'] < C.N_OUT:
            assert not out[name + '_ref32'][:, :, c['P']:].any() and not out[name + '_ref64'][:, :, c['P']:].any()
        assert np.abs(out[name + '_ref64']).max() < 2.0      # the magnitude the accuracy floor assumes


def sampler_cases(out):
    for n in A.SAMPLER_LENGTHS:
        lists = []
        for shuffle in (False, True):
            for epoch in A.SAMPLER_EPOCHS:
                for rank in range(A.SAMPLER_WORLD):
                    s = r_dl.DistributedSampler(A.Sized(n), A.SAMPLER_WORLD, rank, shuffle=shuffle)
                    s.set_epoch(epoch)
                    lists.append(list(iter(s)))
        per_rank = -(-n // A.SAMPLER_WORLD)
        out['sampler_len%d' % n] = np.array(lists, dtype=np.int32).reshape(2, len(A.SAMPLER_EPOCHS), A.SAMPLER_WORLD, per_rank)


if __name__ == '__main__':
    out = {}
    function_cases(out)
    recipe_cases(out)
    sampler_cases(out)
    out['recipe_names'] = np.array(A.recipe_names())
    MG.save('augment.npz', **out)
    size = os.path.getsize(os.path.join(HERE, 'augment.npz'))
    assert size < 400 * 1000, 'the fixture has %d bytes' % size
