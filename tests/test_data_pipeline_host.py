"""CPU: the data pipeline's fixture, the host restatement of its generator, the host-side mirror (cls_wights, Sampler) and
the argument validation of sug_prepare_batch, which happens before any launch."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import data_pipeline_cases as C


@pytest.fixture(scope='module')
def fix():
    return np.load(os.path.join(GOLDEN, 'data_pipeline.npz'), allow_pickle=False)


def test_fixture_keys_and_shapes(fix):
    names = C.case_names()
    assert [str(s) for s in fix['case_names']] == names and len(names) == 24
    M, N = C.CLOUDS_PER_SET, C.N_OUT
    for s, P in C.SHAPES.items():
        assert fix['pts_off_' + s].shape == (M, P, 6) and fix['pts_unit_' + s].shape == (M, P, 3)
        assert fix['pts_off_' + s].dtype == np.float32
        assert fix['noise_' + s].shape == (M, P, 3) and fix['noise_' + s].dtype == np.float32
        assert fix['angle_' + s].shape == (M,) and fix['angle_' + s].dtype == np.float32
        assert (np.abs(fix['noise_' + s]) > 5).sum() >= len(C.PLANTED)            # the clip is exercised
    sel = fix['sel_subset']
    assert sel.shape == (M, N) and sel.min() >= 0 and sel.max() < C.SHAPES['subset']
    assert all(len(set(r.tolist())) == N for r in sel)
    off = fix['pts_off_subset'][:, :, :3]                                           # off-centre, badly scaled
    assert np.abs(off.mean(axis=1)).max() > 0.5 and (off.max(axis=1) - off.min(axis=1)).max() > 2.5
    for name in names:
        c = C.case_of(name)
        r32, r64, dev = fix[name + '_ref32'], fix[name + '_ref64'], float(fix[name + '_dev_ref'])
        assert r32.shape == (M, 3, N) and r32.dtype == np.float32 and r64.shape == (M, 3, N) and r64.dtype == np.float64
        assert dev == np.abs(r32.astype(np.float64) - r64).max() and dev < 1e-5
        if c['P'] < N:
            assert not r32[:, :, c['P']:].any() and not r64[:, :, c['P']:].any()  # padding rows: exact zeros
        if not c['aug']:
            assert abs(np.linalg.norm(r64, axis=1).max() - 1.0) < 1e-6 or c['P'] > N     # normal_pc: largest norm 1
    for key in ('normal_pc', 'rotate_shape_x', 'rotate_shape_y', 'rotate_shape_z', 'rotation_point_cloud', 'jitter_point_cloud',
                'pc_augment', 'random_sample_pc'):
        P_out = N if key == 'random_sample_pc' else C.SHAPES['subset']
        assert fix['fn_%s_ref32' % key].shape == (M, P_out, 3) and fix['fn_%s_ref64' % key].dtype == np.float64, key
        assert float(fix['fn_%s_dev_ref' % key]) < 1e-5
    assert fix['fn_angle'].shape == (1,) and fix['fn_noise'].shape == (C.SHAPES['subset'], 3) and fix['fn_point_idx'].shape == (N,)


def test_philox_known_answers():
    for ctr, key, want in C.PHILOX_KAT:
        got = C.philox4x32_10(np.array(ctr, dtype=np.uint64), key)
        assert [int(v) for v in got] == list(want), (ctr, key)
    # the vectorised form is the scalar one
    w = C._words(7, (3 << 32) | 5, 2, C.DRAW_NOISE, 3)
    one = C.philox4x32_10(np.array([5, 3, 1, C.DRAW_NOISE | 2], dtype=np.uint64), (7, 0))
    assert np.array_equal(w[1, 2], one)


def test_host_draws_are_well_formed():
    sel = C.host_subset(1, 0, 4, 96, 64)
    assert sel.shape == (4, 64) and all(len(set(r.tolist())) == 64 for r in sel) and sel.max() < 96
    ang = C.host_angles(1, 0, 4)
    assert ang.shape == (4,) and (ang >= 0).all() and (ang < 2 * np.pi).all()
    nrm = C.host_normals(1, 0, 4, 64)
    assert nrm.shape == (4, 64, 3) and np.isfinite(nrm).all() and np.abs(nrm).max() < 5.8


def test_cls_wights_equal_the_fixture(fix):
    from sug_amd.data import dataloader as D
    lab = C.labels_list()
    idx = D.class_indices(lab)
    counts = [len(v) for v in idx]
    assert tuple(counts) == C.CLASS_COUNTS
    for i, (w, q) in enumerate(C.WEIGHTINGS):
        got = np.array(D.class_weights(counts, lab.size, w, q), dtype=np.float64)
        assert np.array_equal(got, fix['cls_wights_%d' % i]), (w, q)
        assert abs(got.sum() - 1.0) < 1e-12


def test_sampler_equals_the_fixture(fix):
    from sug_amd.data import dataloader as D
    from sug_amd.utils.train_utils import Sampler
    sampler = Sampler(D.class_indices(C.labels_list()), *C.SAMPLER_ARGS)
    assert len(sampler) == sampler.n_batches == int(fix['sampler_n_batches'][0])
    random.seed(C.SAMPLER_SEED)
    batches = list(iter(sampler))
    assert len(batches) == len(sampler)
    assert np.array_equal(np.array(batches[:C.SAMPLER_BATCHES]), fix['sampler_batches'])


def test_prepare_batch_validates_before_launch():
    from sug_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                # never dereferenced: every call below is refused on the host

    def call(pts=p, M=4, P=64, idx=p, B=2, N=64, stages=1, counter=p, out=p, sel=None):
        rc = L.sug_prepare_batch(pts, M, P, idx, B, N, stages, None, None, None, sel, 0, counter, 0.01, 0.05, out, None, None,
                                 None, None)
        return rc, L.sug_last_error().decode()

    for kw in ({'pts': None}, {'idx': None}, {'out': None}):
        rc, msg = call(**kw)
        assert rc == -1 and 'null' in msg, kw
    rc, msg = call(P=4097, N=4097)
    assert rc == -1 and '4096' in msg
    rc, msg = call(P=64, N=97)
    assert rc == -1 and 'too few points' in msg and '1.5' in msg
    rc, msg = call(B=0)
    assert rc == -1 and 'empty batch' in msg
    rc, msg = call(P=96, N=64, counter=None)              # a subset has to be drawn: the counter is needed
    assert rc == -1 and 'counter' in msg
    rc, msg = call(stages=1 | 2, counter=None)
    assert rc == -1 and 'counter' in msg
    rc, msg = call(P=48, N=64, sel=p)
    assert rc == -1 and 'sel' in msg
    rc, msg = call(stages=64)
    assert rc == -1 and 'stages' in msg


def test_ops_and_dataset_refuse_cpu_tensors():
    from sug_amd import ops
    from sug_amd.data import data_utils, dataloader
    pts = torch.zeros(2, 64, 3)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.prepare_batch(pts, torch.zeros(2, dtype=torch.int32), 64, False, False)
    with pytest.raises(RuntimeError, match='HIP device'):
        data_utils.normal_pc(pts[0])
    with pytest.raises(RuntimeError, match='HIP device'):
        dataloader.UnifiedPointDG('modelnet', pts.numpy(), np.zeros(2, dtype=np.int64), pc_input_num=64, device='cpu')
