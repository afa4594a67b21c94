#!/usr/bin/env python3
"""Generate tests/golden/data_pipeline.npz by RUNNING THE REFERENCE's data/dataloader.py (UnifiedPointDG), data/data_utils.py
and utils/train_utils.py (Sampler) (build container only, CPU).

Usage (from the repo root, a few seconds):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_data_pipeline_goldens.py

Uses make_goldens.py's set-up (stub modules, the reference on sys.path).  Cases and inputs come from
tests/data_pipeline_cases.py, which the tests share.  np.random.uniform / randn / shuffle are wrapped while the reference
runs, so that what it draws is recorded and is exactly representable in fp32 (the kernel takes fp32 draws):
  * uniform() returns a32 / (2 pi) for a recorded fp32 angle a32, so the reference's `uniform() * 2 * pi` is a32 to 1e-15;
  * randn() returns fp32-representable normals with a few planted values beyond +-5 (the clip at 5 sigma acts);
  * shuffle() permutes with the fixture's own generator and the permutation is recorded.
Per case the fixture holds the reference output as fp32 (`ref32`), the same recipe in fp64 on the same fp32 inputs
(`ref64`: the reference's normal_pc / rotation_point_cloud / jitter_point_cloud on float64 input; rotate_shape's product
without its cast to float32) and the reference's own deviation dev_ref = max |ref32 - ref64|."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as MG                 # noqa: E402  (stubs, reference on sys.path)

import data.data_utils as r_du            # noqa: E402  (reference)
import data.dataloader as r_dl            # noqa: E402
import utils.train_utils as r_tu          # noqa: E402

import data_pipeline_cases as C           # noqa: E402


class Draws:
    """Replaces np.random.uniform / randn / shuffle; replays the same draws after reset()."""

    def __init__(self, seed):
        self.seed = seed
        self.reset()

    def reset(self):
        self.rng_u, self.rng_n, self.rng_s = (np.random.RandomState(self.seed + k) for k in range(3))   # one stream per kind
        self.angles, self.noise, self.perms = [], [], []

    def uniform(self):
        a32 = np.float32(self.rng_u.uniform() * 2 * np.pi)
        u = float(a32) / (2 * np.pi)
        assert abs(u * 2 * np.pi - float(a32)) < 1e-14
        self.angles.append(a32)
        return u

    def randn(self, *shape):
        n = self.rng_n.standard_normal(shape).astype(np.float32)
        flat = n.reshape(-1)
        for i, v in enumerate(C.PLANTED):
            flat[(7 + 11 * i) % flat.size] = v
        self.noise.append(n)
        return n.astype(np.float64)

    def shuffle(self, arr):
        self.rng_s.shuffle(arr)
        self.perms.append(arr.copy())

    def __enter__(self):
        self.keep = np.random.uniform, np.random.randn, np.random.shuffle
        np.random.uniform, np.random.randn, np.random.shuffle = self.uniform, self.randn, self.shuffle
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.randn, np.random.shuffle = self.keep


def recipe64(pts, num_points, pre_rotate, aug, angle, noise, perm):
    """UnifiedPointDG.__getitem__ in fp64 on the fp32 inputs, the reference's functions with the recorded draws."""
    x = r_du.normal_pc(pts[:, :3].astype(np.float64))
    if pre_rotate:
        a = -np.pi / 2
        x = x.dot(np.asarray([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]))
    if aug:
        d = Draws(0)
        d.uniform = lambda: float(angle) / (2 * np.pi)
        d.randn = lambda *s: noise.astype(np.float64)
        with d:
            x = r_du.jitter_point_cloud(r_du.rotation_point_cloud(x))
    if x.shape[0] < num_points:
        x = np.concatenate((x, np.zeros((num_points - x.shape[0], 3))), axis=0)
    elif x.shape[0] > num_points:
        x = x[perm[:num_points]]
    return x.transpose()


def getitem_cases(out):
    for s, P in C.SHAPES.items():
        for k, kind in enumerate(C.SETS):
            out['pts_%s_%s' % (kind, s)] = C.make_clouds(kind, P, 100 + 10 * k + P)
    worst = {}
    for name in C.case_names():
        c = C.case_of(name)
        pts = out[c['pts']]
        ds = r_dl.UnifiedPointDG('scannet' if c['pre_rotate'] else 'modelnet', pts, np.zeros(len(pts), dtype=np.int64),
                                 pc_input_num=C.N_OUT, aug=c['aug'], model='DGCNN')
        d = Draws(1000 + c['P'])                       # the same draws for every case of a shape
        ref32, ref64 = [], []
        with d:
            for i in range(len(pts)):
                ref32.append(ds[i][0].numpy()[:, :, 0])
        assert all(r.dtype == np.float32 for r in ref32)
        n_aug, n_perm = (len(pts) if c['aug'] else 0), (len(pts) if c['P'] > C.N_OUT else 0)
        assert len(d.angles) == n_aug and len(d.noise) == n_aug and len(d.perms) == n_perm, name
        for i in range(len(pts)):
            ref64.append(recipe64(pts[i], C.N_OUT, c['pre_rotate'], c['aug'], d.angles[i] if c['aug'] else None,
                                  d.noise[i] if c['aug'] else None, d.perms[i] if n_perm else None))
        ref32, ref64 = np.stack(ref32), np.stack(ref64)
        dev = float(np.abs(ref32.astype(np.float64) - ref64).max())
        assert dev < 1e-4, '%s: the fp64 recipe is not the reference recipe (dev %g)' % (name, dev)
        out[name + '_ref32'], out[name + '_ref64'], out[name + '_dev_ref'] = ref32, ref64, np.float64(dev)
        if c['aug']:                                    # recorded once per shape (every aug case of a shape draws the same)
            angle, noise = np.array(d.angles, dtype=np.float32), np.stack(d.noise)
            assert (np.abs(noise) > 5).sum() >= len(C.PLANTED) and noise.shape == (len(pts), c['P'], 3)
            for key, val in (('angle_' + c['shape'], angle), (c['noise'], noise)):
                assert key not in out or np.array_equal(out[key], val), key
                out[key] = val
        if n_perm:
            sel = np.stack(d.perms)[:, :C.N_OUT].astype(np.int32)
            assert c['sel'] not in out or np.array_equal(out[c['sel']], sel)
            out[c['sel']] = sel
        worst[c['set']] = max(worst.get(c['set'], 0.0), dev)
        print('%-24s dev_ref %.2e' % (name, dev))
    print('largest dev_ref per cloud set:', worst)


def function_cases(out):
    """Each data_utils function alone on 96-point clouds, fp32 input -> output cast to fp32, and fp64: normal_pc on the
    off-centre set (xyz), the others on the unit-scale set (what they see after normal_pc)."""
    pts = out['pts_unit_subset']
    d = Draws(2000)

    def both(key, fn, pts=pts):
        r32, r64 = [], []
        for x in pts:
            d.reset()
            with d:
                r32.append(np.asarray(fn(x)).astype(np.float32))
            d.reset()
            with d:
                r64.append(np.asarray(fn(x.astype(np.float64)), dtype=np.float64))
        r32, r64 = np.stack(r32), np.stack(r64)
        out['fn_%s_ref32' % key], out['fn_%s_ref64' % key] = r32, r64
        out['fn_%s_dev_ref' % key] = np.float64(np.abs(r32.astype(np.float64) - r64).max())
        print('fn %-22s dev_ref %.2e' % (key, out['fn_%s_dev_ref' % key]))

    both('normal_pc', r_du.normal_pc, out['pts_off_subset'][:, :, :3])
    for axis, angle in C.ROTATE_SHAPE_CASES:
        # fp64: rotate_shape casts its result to float32; the fp64 value is its product without the cast
        R = {'x': [[1, 0, 0], [0, np.cos(angle), -np.sin(angle)], [0, np.sin(angle), np.cos(angle)]],
             'y': [[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]],
             'z': [[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]]}[axis]
        r32 = np.stack([r_du.rotate_shape(x, axis, angle) for x in pts])
        r64 = np.stack([x.astype(np.float64).dot(np.asarray(R)) for x in pts])
        assert r32.dtype == np.float32
        out['fn_rotate_shape_%s_ref32' % axis], out['fn_rotate_shape_%s_ref64' % axis] = r32, r64
        out['fn_rotate_shape_%s_dev_ref' % axis] = np.float64(np.abs(r32.astype(np.float64) - r64).max())
    both('rotation_point_cloud', r_du.rotation_point_cloud)
    out['fn_angle'] = np.array(d.angles, dtype=np.float32)
    both('jitter_point_cloud', r_du.jitter_point_cloud)
    out['fn_noise'] = d.noise[0]
    both('pc_augment', r_du.pc_augment)
    assert np.array_equal(out['fn_angle'], np.array(d.angles, dtype=np.float32)) and np.array_equal(out['fn_noise'], d.noise[0])
    both('random_sample_pc', lambda x: r_du.random_sample_pc(x, C.N_OUT))
    out['fn_point_idx'] = d.perms[0][:C.N_OUT].astype(np.int32)


def host_cases(out):
    lab = C.labels_list()
    ds = r_dl.UnifiedPointDG('modelnet', np.zeros((lab.size, 4, 3), dtype=np.float32), lab)
    assert tuple(ds.cls_num_counter) == C.CLASS_COUNTS
    for i, (w, q) in enumerate(C.WEIGHTINGS):
        out['cls_wights_%d' % i] = np.array([float(v) for v in ds.cls_wights(w, q)], dtype=np.float64)
    sampler = r_tu.Sampler(ds.classes(), *C.SAMPLER_ARGS)
    random.seed(C.SAMPLER_SEED)
    batches = list(iter(sampler))
    assert len(batches) >= C.SAMPLER_BATCHES
    out['sampler_batches'] = np.array(batches[:C.SAMPLER_BATCHES], dtype=np.int32)
    out['sampler_n_batches'] = np.array([sampler.n_batches])


if __name__ == '__main__':
    out = {}
    getitem_cases(out)
    function_cases(out)
    host_cases(out)
    out['case_names'] = np.array(C.case_names())
    MG.save('data_pipeline.npz', **out)
    size = os.path.getsize(os.path.join(HERE, 'data_pipeline.npz'))
    assert size < 400 * 1000, 'the fixture has %d bytes' % size
