"""CPU: the augmentation fixture, the rank sharding (DistributedSampler / build_dataloader's host logic) against the
reference's recorded index lists, and the argument validation of sug_prepare_batch_aug, which happens before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import augment_cases as A
import data_pipeline_cases as C


@pytest.fixture(scope='module')
def fix():
    return np.load(os.path.join(GOLDEN, 'augment.npz'), allow_pickle=False)


def test_fixture_keys_and_shapes(fix):
    names = A.recipe_names()
    assert [str(s) for s in fix['recipe_names']] == names and len(names) == 12
    M, N, P = C.CLOUDS_PER_SET, C.N_OUT, A.FN_POINTS
    assert np.array_equal(fix['pts_unit'], A.fn_clouds()) and fix['pts_unit'].shape == (M, P, 3)
    for key in ['fn_' + f for f in A.FUNCTIONS] + ['chain']:
        r32, r64, dev = fix[key + '_ref32'], fix[key + '_ref64'], float(fix[key + '_dev_ref'])
        assert r32.shape == (M, P, 3) and r32.dtype == np.float32 and r64.shape == (M, P, 3) and r64.dtype == np.float64, key
        assert dev == np.abs(r32.astype(np.float64) - r64).max() and dev < 1e-6, key
    assert fix['fn_shifts'].shape == (M, 3) and fix['fn_scales'].shape == (M,) and fix['fn_normals'].shape == (M, 3)
    assert all(fix[k].dtype == np.float32 for k in ('fn_shifts', 'fn_scales', 'fn_normals'))
    assert np.abs(fix['fn_shifts']).max() <= A.SHIFT_RANGE and A.SCALE_LOW <= fix['fn_scales'].min() <= fix['fn_scales'].max() <= A.SCALE_HIGH
    assert fix['fn_normals'][0, 1] == np.float32(A.PLANTED_NORMAL)                 # the clip of the angles is exercised
    # the functions do what their names say (fp64 record against the recorded draws)
    x = fix['pts_unit'].astype(np.float64)
    assert np.abs(fix['fn_shift_point_cloud_ref64'] - (x + fix['fn_shifts'][:, None, :])).max() < 1e-15
    assert np.abs(fix['fn_random_scale_point_cloud_ref64'] - x * fix['fn_scales'][:, None, None]).max() < 1e-15
    norms = np.linalg.norm(fix['fn_rotate_perturbation_point_cloud_ref64'], axis=2)
    assert np.abs(norms - np.linalg.norm(x, axis=2)).max() < 1e-14                  # a rotation
    shapes = {'angle': (M,), 'scales': (M,), 'normals': (M, 3), 'shifts': (M, 3)}
    for prefix, Pc in [('chain_%s', P)] + [('%%s_%s' % s, Ps) for s, Ps in C.SHAPES.items()]:
        for k, shp in shapes.items():
            assert fix[prefix % k].shape == shp and fix[prefix % k].dtype == np.float32, prefix % k
        assert fix[prefix % 'noise'].shape == (M, Pc, 3) and fix[prefix % 'noise'].dtype == np.float32
    sel = fix['sel_subset']
    assert sel.shape == (M, N) and sel.min() >= 0 and sel.max() < C.SHAPES['subset']
    assert all(len(set(r.tolist())) == N for r in sel)
    for name in names:
        c = A.recipe_of(name)
        assert np.array_equal(fix[c['pts']], A.recipe_clouds(c['set'], c['shape']))
        r32, r64, dev = fix[name + '_ref32'], fix[name + '_ref64'], float(fix[name + '_dev_ref'])
        assert r32.shape == (M, 3, N) and r32.dtype == np.float32 and r64.shape == (M, 3, N) and r64.dtype == np.float64
        assert dev == np.abs(r32.astype(np.float64) - r64).max() and dev < 1e-5
        assert np.abs(r64).max() < 2.0                                              # what the accuracy floor assumes
        if c['P'] < N:
            assert not r32[:, :, c['P']:].any() and not r64[:, :, c['P']:].any()  # padding rows: exact zeros, unshifted


def test_host_draws_are_well_formed():
    s = A.host_scales(1, 0, 64)
    assert s.shape == (64,) and (s >= A.SCALE_LOW).all() and (s < A.SCALE_HIGH).all() and len(set(s.tolist())) == 64
    t = A.host_shifts(1, 0, 64)
    assert t.shape == (64, 3) and (t >= -A.SHIFT_RANGE).all() and (t < A.SHIFT_RANGE).all()
    n = A.host_perturb_normals(1, 0, 64)
    assert n.shape == (64, 3) and np.isfinite(n).all() and np.abs(n).max() < 5.8
    # the block of each purpose is its own: index 0 of the perturbation purpose is not noise row 0
    assert not np.allclose(n, C.host_normals(1, 0, 64, 1)[:, 0])


@pytest.mark.parametrize('n', A.SAMPLER_LENGTHS)
def test_distributed_sampler_equals_the_fixture(fix, n):
    from sug_amd.data.dataloader import DistributedSampler
    want = fix['sampler_len%d' % n]
    per_rank = -(-n // A.SAMPLER_WORLD)
    assert want.shape == (2, len(A.SAMPLER_EPOCHS), A.SAMPLER_WORLD, per_rank)
    for si, shuffle in enumerate((False, True)):
        for ei, epoch in enumerate(A.SAMPLER_EPOCHS):
            seen = []
            for rank in range(A.SAMPLER_WORLD):
                s = DistributedSampler(A.Sized(n), num_replicas=A.SAMPLER_WORLD, rank=rank, shuffle=shuffle)
                s.set_epoch(epoch)
                got = list(s)
                assert len(s) == per_rank and got == want[si, ei, rank].tolist(), (n, shuffle, epoch, rank)
                seen += got
            assert sorted(set(seen)) == list(range(n)) and len(seen) == per_rank * A.SAMPLER_WORLD   # every index, padded by wrapping
    assert not np.array_equal(want[1, 0], want[1, 1])                                # set_epoch changes the order
    assert np.array_equal(want[0, 0], want[0, 1])                                    # ... of the shuffled sampler only


def test_distributed_sampler_defaults_need_a_process_group():
    from sug_amd.data.dataloader import DistributedSampler
    from sug_amd.utils.common_utils import get_dist_info
    assert get_dist_info() == (0, 1) and len(get_dist_info(return_gpu_per_machine=True)) == 3
    with pytest.raises((RuntimeError, ValueError)):
        DistributedSampler(A.Sized(10))                    # as torch's: rank and world size come from the process group


def test_loader_refuses_sampler_with_shuffle():
    from sug_amd.data.dataloader import DeviceLoader, DistributedSampler

    class Stub(A.Sized):
        seed = 0
    s = DistributedSampler(Stub(10), 3, 0)
    with pytest.raises(ValueError, match='mutually exclusive'):
        DeviceLoader(Stub(10), batch_size=2, shuffle=True, sampler=s)
    with pytest.raises(ValueError, match='mutually exclusive'):
        DeviceLoader(Stub(10), batch_sampler=[[0, 1]], sampler=s)
    loader = DeviceLoader(Stub(10), batch_size=3, sampler=s, drop_last=True)
    assert len(loader) == 1 and len(DeviceLoader(Stub(10), batch_size=3, sampler=s)) == 2      # of this rank's 4 indices


def test_parse_aug():
    from sug_amd import ops
    from sug_amd.data.dataloader import parse_aug
    stages, kw = parse_aug({'rotate_z': True, 'jitter': (0.01, 0.05), 'scale': (0.8, 1.25), 'perturb': (0.06, 0.18), 'shift': 0.1})
    assert stages == ops.PREP_ROTATE_Z | ops.PREP_JITTER | ops.PREP_SCALE | ops.PREP_PERTURB | ops.PREP_SHIFT
    assert kw == {'sigma': 0.01, 'clip': 0.05, 'scale_low': 0.8, 'scale_high': 1.25, 'angle_sigma': 0.06, 'angle_clip': 0.18,
                  'shift_range': 0.1}
    assert parse_aug({}) == (0, {}) and parse_aug({'shift': False, 'rotate_z': None}) == (0, {})       # missing / off
    assert parse_aug({'scale': True}) == (ops.PREP_SCALE, {'scale_low': A.SCALE_LOW, 'scale_high': A.SCALE_HIGH})
    with pytest.raises(ValueError, match="'dropout'"):
        parse_aug({'shift': 0.1, 'dropout': 0.5})


def test_prepare_batch_aug_validates_before_launch():
    from sug_amd import _lib, ops
    L = _lib.lib()
    p = ctypes.c_void_p(256)                # never dereferenced: every call below is refused on the host
    ALL = ops.PREP_SCALE | ops.PREP_PERTURB | ops.PREP_SHIFT

    def call(stages=1 | ALL, params=(0.8, 1.25, 0.1, 0.06, 0.18), counter=p, scales=None, perturb=None, shifts=None, pts=p, P=64,
             N=64, no_params=False):
        arr = None if no_params else (ctypes.c_float * ops.PREP_AUG_PARAMS)(*params)
        rc = L.sug_prepare_batch_aug(pts, 4, P, p, 2, N, stages, None, None, None, None, scales, perturb, shifts, 0, counter, 0.01,
                                     0.05, arr, p, None, None, None, None, None, None, None)
        return rc, L.sug_last_error().decode()

    rc, msg = call(params=(1.3, 1.25, 0.1, 0.06, 0.18))
    assert rc == -1 and 'sug_prepare_batch_aug' in msg and 'scale_low' in msg and 'scale_high' in msg
    for bad in (0.0, -0.8, float('nan')):
        rc, msg = call(params=(bad, 1.25, 0.1, 0.06, 0.18))
        assert rc == -1 and 'scale_low' in msg, bad
    rc, msg = call(params=(0.8, float('inf'), 0.1, 0.06, 0.18))
    assert rc == -1 and 'scale_high' in msg
    rc, msg = call(params=(0.8, 1.25, -0.1, 0.06, 0.18))
    assert rc == -1 and 'shift_range' in msg
    rc, msg = call(params=(0.8, 1.25, 0.1, -0.06, 0.18))
    assert rc == -1 and 'angle_sigma' in msg
    rc, msg = call(params=(0.8, 1.25, 0.1, 0.06, -0.18))
    assert rc == -1 and 'angle_clip' in msg
    rc, msg = call(no_params=True)
    assert rc == -1 and 'aug_params' in msg
    # a null counter with a drawn stage: each new stage alone, its draw not supplied
    for bit, kw in ((ops.PREP_SCALE, {'perturb': p, 'shifts': p}), (ops.PREP_PERTURB, {'scales': p, 'shifts': p}),
                    (ops.PREP_SHIFT, {'scales': p, 'perturb': p})):
        rc, msg = call(stages=1 | bit, counter=None, **kw)
        assert rc == -1 and 'counter' in msg, bit
    rc, msg = call(stages=1 | 2, counter=None)                                      # the old stages as before
    assert rc == -1 and 'counter' in msg
    rc, msg = call(stages=128)
    assert rc == -1 and 'stages' in msg and 'sug_prepare_batch_aug' in msg
    rc, msg = call(pts=None)
    assert rc == -1 and 'null' in msg
    rc, msg = call(P=4097, N=4097)
    assert rc == -1 and '4096' in msg
    # the old entry point keeps refusing the new bits
    rc = L.sug_prepare_batch(p, 4, 64, p, 2, 64, ops.PREP_SHIFT, None, None, None, None, 0, p, 0.01, 0.05, p, None, None, None, None)
    assert rc == -1 and 'stages' in L.sug_last_error().decode()


def test_header_constants_equal_ops():
    from sug_amd import _lib, ops
    H = _lib.CONSTANTS
    assert (ops.PREP_SCALE, ops.PREP_PERTURB, ops.PREP_SHIFT) == (H['SUG_PREP_SCALE'], H['SUG_PREP_PERTURB'], H['SUG_PREP_SHIFT']) \
        == (16, 32, 64)
    assert (H['SUG_PREP_DRAW_SCALE'], H['SUG_PREP_DRAW_PERTURB'], H['SUG_PREP_DRAW_SHIFT']) == (A.DRAW_SCALE, A.DRAW_PERTURB, A.DRAW_SHIFT)
    assert (H['SUG_PREP_DRAW_ANGLE'], H['SUG_PREP_DRAW_SUBSET'], H['SUG_PREP_DRAW_NOISE']) == (C.DRAW_ANGLE, C.DRAW_SUBSET, C.DRAW_NOISE)
    assert ops.PREP_AUG_PARAMS == H['SUG_PREP_AUG_PARAMS'] == 5
    assert sorted(H['SUG_PREP_AUG_' + n] for n in ('SCALE_LOW', 'SCALE_HIGH', 'SHIFT_RANGE', 'ANGLE_SIGMA', 'ANGLE_CLIP')) == list(range(5))
    assert H['SUG_ABI_VERSION'] == 8                                                # additive: the version does not move
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.DECLARATIONS['sug_prepare_batch_aug'] == (ctypes.c_int, [P, I, I, P, I, I, I] + [P] * 7 + [ctypes.c_uint64, P, F, F, P]
                                                          + [P] * 8)


def test_ops_and_data_utils_refuse_cpu_tensors():
    from sug_amd import ops
    from sug_amd.data import data_utils as DU
    pts = torch.zeros(2, 64, 3)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.prepare_batch_aug(pts, torch.zeros(2, dtype=torch.int32), 64, False, False, stages=ops.PREP_SHIFT)
    for fn in (DU.shift_point_cloud, DU.random_scale_point_cloud, DU.rotate_perturbation_point_cloud,
               lambda x: DU.rotate_point_cloud_by_angle(x, 0.3), lambda x: DU.fps(x, 8),
               lambda x: DU.pc_augment(x, scale=True, perturb=True, shift=True)):
        with pytest.raises(RuntimeError, match='HIP device'):
            fn(pts[0])
    with pytest.raises(RuntimeError, match='HIP device'):
        DU.farthest_point_sample(pts.transpose(1, 2), 8)
