"""GPU: the scale / rotation-perturbation / shift stages of the data pipeline (sug_prepare_batch_aug, the data_utils
functions over it, UnifiedPointDG(aug={...})) against the reference's functions recorded in tests/golden/augment.npz, the
three new in-kernel draws against their host restatement in tests/augment_cases.py, and the rank sharding of DeviceLoader.

Accuracy rule of the parity tests (the data pipeline's): the kernel's max-abs deviation from the fp64 recipe must not exceed
the larger of twice the reference's own fp32-vs-fp64 deviation of that case (`dev_ref`) and a floor, and never 1e-4.

The floor.  Every coordinate stays below 2 in magnitude (at most 1.25 * (1 + 0.05 * sqrt(3)) + 0.1; the fixture asserts it),
so one fp32 rounding moves it by at most 2^-24 (half an ulp of [1, 2)); floor = R * 2^-24 with R the number of fp32
roundings that reach one output coordinate through the enabled stages.  The library is built with -ffp-contract=off: a
product and a sum are two roundings.  The reference works in float64 from its first rotation on, so each of these is
the kernel's alone.  Stage by stage (ROUNDINGS below):
  normalise      6   the centred coordinate (fp64 difference rounded once), its division by the largest norm; that norm is
                     sqrtf of a sum of three squares (5 roundings, halved by the root, and the root's own: at most 3.5
                     relative roundings on a coordinate of at most 1) -> 4
  pre-rotation   8   (x R0j + y R1j) + z R2j: 3 products, 2 sums; the three fp32 matrix entries, rounded from fp64 on the
                     host, each at most one rounding of a term below 2
  z-rotation     7   x c + y s: 2 products, 1 sum; c and s from sincosf of the fp32 angle, allowed 2 ulp each -> 4
  jitter         2   sigma * n, the sum (the clip is exact)
  scale          1   one product by the supplied fp32 factor
  perturbation   9   3 products, 2 sums; the three entries of R, formed in fp64 and rounded once -> 3; the fp32
                     angle_sigma / angle_clip against the reference's doubles: a relative 2^-25 on three angles of at
                     most 0.18 each turning a coordinate below 2 -> at most 0.54 * 2^-24 -> 1
  shift          1   one sum with the supplied fp32 component
All five stages behind normalise and the pre-rotation: R = 34, floor 2.03e-6; a function alone has its own R (scale: 1, 6e-8).
Measured on an MI355X: DESIGN section 10a's parity table."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import augment_cases as A
import data_pipeline_cases as C

pytestmark = pytest.mark.gpu

SEED = 0x1234567887654321
ROUNDINGS = {'normalize': 6, 'pre': 8, 'rotate_z': 7, 'jitter': 2, 'scale': 1, 'perturb': 9, 'shift': 1}
FIVE = ('rotate_z', 'jitter', 'scale', 'perturb', 'shift')
PARAMS = dict(scale_low=A.SCALE_LOW, scale_high=A.SCALE_HIGH, shift_range=A.SHIFT_RANGE, angle_sigma=A.ANGLE_SIGMA,
              angle_clip=A.ANGLE_CLIP)


def floor(*stages):
    return sum(ROUNDINGS[s] for s in stages) * 2.0 ** -24


def bound(dev_ref, *stages):
    return min(max(2.0 * float(dev_ref), floor(*stages)), 1e-4)


@pytest.fixture(scope='module')
def fix():
    return np.load(os.path.join(GOLDEN, 'augment.npz'), allow_pickle=False)


def cu(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def counter_t(v=0):
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v], dtype=torch.int64, device='cuda')


def arange_idx(B):
    return torch.arange(B, dtype=torch.int32, device='cuda')


def bits(ops, *stages):
    table = {'normalize': ops.PREP_NORMALIZE, 'rotate_z': ops.PREP_ROTATE_Z, 'jitter': ops.PREP_JITTER, 'scale': ops.PREP_SCALE,
             'perturb': ops.PREP_PERTURB, 'shift': ops.PREP_SHIFT}
    return sum(table[s] for s in stages)


def check_parity(fix, key, got, stages):
    got = got.cpu().numpy().astype(np.float64)
    ref64, dev_ref = fix[key + '_ref64'], float(fix[key + '_dev_ref'])
    assert got.shape == ref64.shape, key
    dev, lim = np.abs(got - ref64).max(), bound(dev_ref, *stages)
    print('%s: kernel dev %.3e, dev_ref %.3e, bound %.3e' % (key, dev, dev_ref, lim))
    assert dev <= lim, '%s: %.3e > %.3e (dev_ref %.3e)' % (key, dev, lim, dev_ref)


def supplied(fix, prefix):
    """The recorded draws '<prefix>_...' / '..._<shape>' as prepare_batch_aug's keywords."""
    return {'angles': cu(fix[prefix % 'angle']), 'noise': cu(fix[prefix % 'noise']), 'scales': cu(fix[prefix % 'scales']),
            'perturb': cu(fix[prefix % 'normals']), 'shifts': cu(fix[prefix % 'shifts'])}


# ------------------------------------------------------------------------------------------------ 1. parity, supplied draws
@pytest.mark.parametrize('fn,stage,kw,key', [('shift_point_cloud', 'shift', 'shifts', 'fn_shifts'),
                                             ('random_scale_point_cloud', 'scale', 'scales', 'fn_scales'),
                                             ('rotate_perturbation_point_cloud', 'perturb', 'perturb', 'fn_normals')])
def test_parity_each_stage_alone(fix, fn, stage, kw, key):
    from sug_amd import ops
    pts = cu(fix['pts_unit'])
    out = ops.prepare_batch_aug(pts, arange_idx(len(pts)), pts.shape[1], False, False, stages=bits(ops, stage), **PARAMS,
                                **{kw: cu(fix[key])})
    check_parity(fix, 'fn_' + fn, out.transpose(1, 2), (stage,))


def test_parity_five_stage_chain(fix):
    from sug_amd import ops
    pts = cu(fix['pts_unit'])
    out = ops.prepare_batch_aug(pts, arange_idx(len(pts)), pts.shape[1], False, False, stages=bits(ops, *FIVE), sigma=C.SIGMA,
                                clip=C.CLIP, **PARAMS, **supplied(fix, 'chain_%s'))
    check_parity(fix, 'chain', out.transpose(1, 2), FIVE)


@pytest.mark.parametrize('name', A.recipe_names())
def test_parity_full_recipe(fix, name):
    from sug_amd import ops
    c = A.recipe_of(name)
    pts = cu(fix[c['pts']][:, :, :3])
    kw = supplied(fix, '%s_' + c['shape'])
    if c['P'] > C.N_OUT:
        kw['sel'] = cu(fix['sel_' + c['shape']])
    out = ops.prepare_batch_aug(pts, arange_idx(len(pts)), C.N_OUT, c['pre_rotate'], True, stages=bits(ops, 'normalize', *FIVE),
                                sigma=C.SIGMA, clip=C.CLIP, **PARAMS, **kw)
    assert out.shape == (len(pts), 3, C.N_OUT) and out.dtype == torch.float32
    check_parity(fix, name, out, ('normalize',) + (('pre',) if c['pre_rotate'] else ()) + FIVE)
    if c['P'] < C.N_OUT:
        assert not out[:, :, c['P']:].cpu().numpy().any(), 'padding rows are not exact zeros'


# ------------------------------------------------------------------------------------------------ 2. padding rows
def test_padding_rows_stay_exact_zeros():
    from sug_amd import ops
    B, P, N = 4, 48, 64
    pts = torch.rand(B, P, 3, generator=torch.Generator().manual_seed(3)).cuda()
    out, *_, sh = ops.prepare_batch_aug(pts, arange_idx(B), N, True, True, stages=bits(ops, 'normalize', *FIVE), seed=SEED,
                                        counter=counter_t(9), return_draws=True, **PARAMS)
    assert bool((sh.abs() > 1e-4).any(dim=1).all()), 'every cloud is shifted'
    assert not out[:, :, P:].cpu().numpy().any(), 'a shift, scale or rotation reached the padding rows'
    assert bool((out[:, :, :P] != 0).all())


# ------------------------------------------------------------------------------------------------ 3. new stages off
@pytest.mark.parametrize('P,N', [(96, 64), (48, 64), (100, 75)])
def test_new_stages_off_equals_prepare_batch(P, N):
    from sug_amd import ops
    B = 3
    g = torch.Generator().manual_seed(P)
    pts = torch.rand(B, P, 3, generator=g).cuda()
    idx = torch.tensor([2, 0, 2], dtype=torch.int32, device='cuda')
    kw = {'angles': (torch.rand(B, generator=g) * 6.28).cuda(), 'noise': torch.randn(B, P, 3, generator=g).cuda()}
    if P > N:
        kw['sel'] = torch.stack([torch.randperm(P, generator=g)[:N] for _ in range(B)]).to(torch.int32).cuda()
    old = ops.prepare_batch(pts, idx, N, True, True, **kw)
    assert torch.equal(ops.prepare_batch_aug(pts, idx, N, True, True, **kw), old)
    old = ops.prepare_batch(pts, idx, N, True, True, seed=SEED, counter=counter_t(7), return_draws=True)
    new = ops.prepare_batch_aug(pts, idx, N, True, True, seed=SEED, counter=counter_t(7), return_draws=True)
    for x, y in zip(old, new[:4]):
        assert torch.equal(x, y)
    sc, pn, sh = new[4:]
    assert bool((sc == 1).all()) and not pn.cpu().numpy().any() and not sh.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ 4. in-kernel draws, fed back
@pytest.mark.parametrize('shape', list(C.SHAPES))
def test_in_kernel_draws_transform(fix, shape):
    from sug_amd import ops
    pts = cu(fix['pts_unit_' + shape])
    B, P, N = pts.shape[0], C.SHAPES[shape], C.N_OUT
    stages = bits(ops, 'normalize', *FIVE)
    out, ang, nz, sel, sc, pn, sh = ops.prepare_batch_aug(pts, arange_idx(B), N, True, True, stages=stages, seed=SEED,
                                                          counter=counter_t(5), return_draws=True, **PARAMS)
    assert ang.shape == (B,) and nz.shape == (B, N, 3) and sel.shape == (B, N)
    assert sc.shape == (B,) and pn.shape == (B, 3) and sh.shape == (B, 3)
    assert all(t.dtype == torch.float32 for t in (sc, pn, sh))
    noise = torch.zeros(B, P, 3, device='cuda')                 # per-kept-point noise back to its point position
    if P >= N:
        noise.scatter_(1, sel.long().unsqueeze(-1).expand(-1, -1, 3), nz)
    else:
        noise[:, :P] = nz[:, :P]
    kw = {'sel': sel.contiguous()} if P > N else {}
    again = ops.prepare_batch_aug(pts, arange_idx(B), N, True, True, stages=stages, angles=ang, noise=noise, scales=sc, perturb=pn,
                                  shifts=sh, **PARAMS, **kw)
    assert torch.equal(out, again)


# ------------------------------------------------------------------------------------------------ 5. the generator
@pytest.mark.parametrize('P,N,seed,ctr', [(96, 64, SEED, 5), (100, 75, 1, 1), (4096, 3000, 2 ** 63 + 11, 0)])
def test_generator_matches_host_restatement(P, N, seed, ctr):
    from sug_amd import ops
    B = 3
    pts = torch.rand(B, P, 3, generator=torch.Generator().manual_seed(P)).cuda()
    idx = torch.tensor([2, 0, 2], dtype=torch.int32, device='cuda')
    _, ang, nz, sel, sc, pn, sh = ops.prepare_batch_aug(pts, idx, N, False, True, stages=bits(ops, 'normalize', *FIVE), seed=seed,
                                                        counter=counter_t(ctr), return_draws=True, **PARAMS)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    assert np.abs(f64(sc) - A.host_scales(seed, ctr, B)).max() <= 1e-6
    assert np.abs(f64(sh) - A.host_shifts(seed, ctr, B)).max() <= 1e-6
    assert np.abs(f64(pn) - A.host_perturb_normals(seed, ctr, B)).max() <= 1e-5
    # the old draws of the same launch have not moved
    assert np.array_equal(sel.cpu().numpy(), C.host_subset(seed, ctr, B, P, N))
    assert np.abs(f64(ang) - C.host_angles(seed, ctr, B)).max() <= 1e-6
    assert np.abs(f64(nz) - C.host_normals(seed, ctr, B, N)).max() <= 1e-5


def _angles_of(R):
    """The three angles of R = Rz (Ry Rx) [.., 3, 3] (data_utils.py:154-163): R20 = -sin y, R21 / R22 = tan x, R10 / R00 = tan z."""
    return np.stack([np.arctan2(R[..., 2, 1], R[..., 2, 2]), -np.arcsin(R[..., 2, 0]), np.arctan2(R[..., 1, 0], R[..., 0, 0])], axis=-1)


def test_generator_distribution():
    """One fixed seed, B = 64 x 4 batches; every bound is six standard deviations of the statistic under the null.  The
    perturbation angles are read off the kernel's own matrix: the stage alone applied to the three unit vectors writes R."""
    from sug_amd import ops
    B = 64
    eye = torch.eye(3).reshape(1, 3, 3).cuda()
    pts = torch.rand(1, 64, 3, generator=torch.Generator().manual_seed(0)).cuda()
    idx = torch.zeros(B, dtype=torch.int32, device='cuda')
    sigma, clip = 0.06, 0.09                                   # the clip at 1.5 sigma: 13% of the angles pile up there
    scs, shs, angs = [], [], []
    for step in range(4):
        _, _, _, _, sc, _, sh = ops.prepare_batch_aug(pts, idx, 64, False, False, stages=bits(ops, 'scale', 'shift'), seed=2024,
                                                      counter=counter_t(step), return_draws=True, **PARAMS)
        scs.append(sc.cpu().numpy().astype(np.float64)), shs.append(sh.cpu().numpy().astype(np.float64))
        out, _, _, _, _, pn, _ = ops.prepare_batch_aug(eye, idx, 3, False, False, stages=bits(ops, 'perturb'), seed=2024,
                                                       counter=counter_t(step), return_draws=True, angle_sigma=sigma, angle_clip=clip)
        R = out.cpu().numpy().astype(np.float64).transpose(0, 2, 1)          # out[b, j, n] = (e_n . R)_j = R[n, j]
        a = _angles_of(R)
        want = np.clip(sigma * pn.cpu().numpy().astype(np.float64), -clip, clip)
        assert np.abs(a - want).max() <= 1e-6, 'the matrix is not Rz (Ry Rx) of the clipped angles'
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
        angs.append(a)
    u = (np.concatenate(scs) - A.SCALE_LOW) / (A.SCALE_HIGH - A.SCALE_LOW)
    v = (np.concatenate(shs).reshape(-1) + A.SHIFT_RANGE) / (2 * A.SHIFT_RANGE)
    for w, m in ((u, 256), (v, 768)):
        assert w.size == m and (w >= 0).all() and (w <= 1).all()
        assert abs(w.mean() - 0.5) <= 6 * np.sqrt(1.0 / 12.0 / m)
        h = np.histogram(w, bins=8, range=(0, 1))[0] / m
        assert np.abs(h - 0.125).max() <= 6 * np.sqrt(0.125 * 0.875 / m)
    a = np.concatenate(angs).reshape(-1)
    m, al = a.size, clip / sigma
    assert m == 768 and np.abs(a).max() <= clip + 1e-6
    phi, Z = math.exp(-al * al / 2) / math.sqrt(2 * math.pi), math.erf(al / math.sqrt(2))     # density at the cut, mass inside
    at_clip = np.abs(a) >= clip - 1e-6
    assert abs(at_clip.mean() - (1 - Z)) <= 6 * np.sqrt(Z * (1 - Z) / m)
    assert abs((a[at_clip] > 0).mean() - 0.5) <= 6 * np.sqrt(0.25 / at_clip.sum())           # both ends
    z = a[~at_clip] / sigma                                    # the truncated standard normal on (-al, al)
    k = z.size
    m2 = 1 - 2 * al * phi / Z
    m4 = 3 * m2 - 2 * al ** 3 * phi / Z
    assert abs(z.mean()) <= 6 * np.sqrt(m2 / k)
    assert abs((z ** 2).mean() - m2) <= 6 * np.sqrt((m4 - m2 * m2) / k)


# ------------------------------------------------------------------------------------------------ 7. determinism, counters
def test_determinism_and_counters():
    from sug_amd import ops
    N = 64
    pts = torch.rand(3, 96, 3, generator=torch.Generator().manual_seed(1)).cuda()
    idx = torch.tensor([0, 1, 2, 1, 1, 0, 2, 2], dtype=torch.int32, device='cuda')
    run = lambda c, seed=SEED: ops.prepare_batch_aug(pts, idx, N, True, True, stages=bits(ops, 'normalize', *FIVE), seed=seed,
                                                     counter=counter_t(c), return_draws=True, **PARAMS)
    a, b, nxt = run(41), run(41), run(42)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert bool((a[4] != nxt[4]).all()), 'counter + 1 must change every scale'
    assert bool((a[5] != nxt[5]).all()), 'counter + 1 must change every perturbation draw'
    assert bool((a[6] != nxt[6]).all()), 'counter + 1 must change every shift'
    # clouds 1, 3, 4 of the batch are the same dataset cloud: different draws all the same
    for i, j in ((1, 3), (1, 4), (3, 4), (0, 5)):
        assert a[4][i] != a[4][j] and bool((a[5][i] != a[5][j]).all()) and bool((a[6][i] != a[6][j]).all())
        assert not torch.equal(a[0][i], a[0][j])
    other = run(41, SEED + 1)
    assert bool((a[4] != other[4]).all()) and bool((a[6] != other[6]).all())


# ------------------------------------------------------------------------------------------------ 8. graph capture
def test_graph_capture_replays_with_fresh_draws():
    from sug_amd import ops
    B, P, N, M = 8, 96, 64, 20
    pts = torch.rand(M, P, 3, generator=torch.Generator().manual_seed(2)).cuda()
    idx = arange_idx(B)
    cnt = counter_t(100)
    out = torch.empty(B, 3, N, device='cuda')
    kw = dict(stages=bits(ops, 'normalize', *FIVE), seed=SEED, **PARAMS)
    ops.prepare_batch_aug(pts, idx, N, True, True, counter=cnt, out=out, **kw)        # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.prepare_batch_aug(pts, idx, N, True, True, counter=cnt, out=out, **kw)
    seen = []
    for r in range(3):
        idx.copy_(torch.tensor([(3 * r + 2 * i) % M for i in range(B)], dtype=torch.int32))
        cnt.add_(1)
        graph.replay()
        eager = ops.prepare_batch_aug(pts, idx.clone(), N, True, True, counter=cnt.clone(), **kw)
        assert torch.equal(out, eager), 'replay %d differs from the eager call' % r
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ------------------------------------------------------------------------------------------------ 9. data_utils
def test_data_utils_functions(fix):
    from sug_amd.data import data_utils as DU
    unit = cu(fix['pts_unit'])
    B, P, _ = unit.shape
    keep = unit.clone()
    shifts, scales, normals = cu(fix['fn_shifts']), cu(fix['fn_scales']), cu(fix['fn_normals'])
    runs = {
        'shift_point_cloud': (lambda x, i=slice(None): DU.shift_point_cloud(x, shifts=shifts[i]), 'shift'),
        'random_scale_point_cloud': (lambda x, i=slice(None): DU.random_scale_point_cloud(x, scales=scales[i]), 'scale'),
        'rotate_perturbation_point_cloud': (lambda x, i=slice(None): DU.rotate_perturbation_point_cloud(x, normals=normals[i]), 'perturb'),
    }
    for key, (fn, stage) in runs.items():
        got = fn(unit)
        check_parity(fix, 'fn_' + key, got, (stage,))
        one = fn(unit[1], 1)                                   # one cloud [P, 3] in, one cloud out
        assert one.shape == (P, 3) and torch.equal(one, got[1]), key
    ch = supplied(fix, 'chain_%s')
    got = DU.pc_augment(unit, angle=ch['angles'], noise=ch['noise'], scale=True, perturb=True, shift=True, scales=ch['scales'],
                        normals=ch['perturb'], shifts=ch['shifts'])
    check_parity(fix, 'chain', got, FIVE)
    assert torch.equal(DU.pc_augment(unit, angle=ch['angles'], noise=ch['noise']),             # the switches default to off
                       DU.jitter_point_cloud(DU.rotation_point_cloud(unit, angle=ch['angles']), noise=ch['noise']))
    # rotate_point_cloud_by_angle: the y-axis matrix, against the fp64 product (bound: a rotation by an fp32 matrix)
    ang = 0.7
    c, s = math.cos(ang), math.sin(ang)
    want = fix['pts_unit'].astype(np.float64) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    got = DU.rotate_point_cloud_by_angle(unit, ang)
    assert np.abs(got.cpu().numpy().astype(np.float64) - want).max() <= floor('pre')
    assert torch.equal(got, DU.rotate_shape(unit, 'y', ang))
    # the generator path: reproducible after manual_seed, advancing between calls, every function drawing
    for fn in (DU.shift_point_cloud, DU.random_scale_point_cloud, DU.rotate_perturbation_point_cloud,
               lambda x: DU.pc_augment(x, scale=True, perturb=True, shift=True)):
        DU.manual_seed(3)
        a1, a2 = fn(unit), fn(unit)
        DU.manual_seed(3)
        assert torch.equal(a1, fn(unit)) and not torch.equal(a1, a2) and not torch.equal(a1, unit)
        assert a1.shape == unit.shape and not torch.equal(a1[0] - unit[0], a1[1] - unit[1])    # one draw per cloud
    lo = DU.random_scale_point_cloud(unit, 2.0, 2.0)            # scale_low == scale_high: the factor itself
    assert torch.equal(lo, unit * 2.0)
    assert torch.equal(unit, keep), 'an argument was mutated'


def test_data_utils_fps(fix):
    from sug_amd import ops
    from sug_amd.data import data_utils as DU
    from sug_amd.dataset_splitter import process_pts
    pts = cu(fix['pts_off_subset'][:, :, :3])
    want, idx = process_pts(pts, pt_num=20, return_index=True)
    normal = DU.normal_pc(pts)
    got = DU.fps(normal, 20)
    assert got.shape == (pts.shape[0], 20, 3) and torch.equal(got, want)
    assert torch.equal(got, torch.gather(normal, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))) and bool((idx[:, 0] == 0).all())
    assert torch.equal(DU.fps(normal[1], 20), got[1])
    # farthest_point_sample: the start from torch.randint on the host generator, then the FPS kernel
    xyz = normal.transpose(1, 2).contiguous()                 # [B, C, N]
    torch.manual_seed(5)
    cent, vals = DU.farthest_point_sample(xyz, 16)
    torch.manual_seed(5)
    start = torch.randint(0, xyz.shape[2], (xyz.shape[0],), dtype=torch.long)
    assert cent.dtype == torch.int64 and cent.shape == (xyz.shape[0], 16) and vals.shape == (xyz.shape[0], 3, 16)
    assert torch.equal(cent[:, 0].cpu(), start)
    assert torch.equal(cent, ops.fps(normal.contiguous(), 16, start).long())
    assert torch.equal(vals, torch.gather(xyz, 2, cent.unsqueeze(1).expand(-1, 3, -1)))
    assert all(len(set(r.tolist())) == 16 for r in cent.cpu())


# ------------------------------------------------------------------------------------------------ 10. dataset and loader
ALL_ON = {'rotate_z': True, 'jitter': (0.01, 0.05), 'scale': (0.8, 1.25), 'perturb': (0.06, 0.18), 'shift': 0.1}


def _dataset(M=40, P=96, N=64, aug=False, seed=0, **kw):
    from sug_amd.data.dataloader import UnifiedPointDG
    g = torch.Generator().manual_seed(11)
    pts = (torch.rand(M, P, 3, generator=g) * 2 - 1).numpy()
    labels = torch.randint(0, 10, (M,), generator=g).numpy()
    return UnifiedPointDG('scannet', pts, labels, pc_input_num=N, aug=aug, seed=seed, **kw), pts, labels


def test_dataset_with_a_stage_mapping():
    from sug_amd import ops
    from sug_amd.data.dataloader import DeviceLoader, UnifiedPointDG
    ds, pts, labels = _dataset(aug=ALL_ON, seed=5)
    batches = list(DeviceLoader(ds, batch_size=16, shuffle=False))
    assert [b[0].shape for b in batches] == [(16, 3, 64, 1), (16, 3, 64, 1), (8, 3, 64, 1)]
    assert all(d.dtype == torch.float32 and d.is_cuda and l.dtype == torch.int64 and l.is_cuda for d, l in batches)
    assert np.array_equal(torch.cat([l for _, l in batches]).cpu().numpy(), labels)
    assert int(ds.counter) == 3                                 # one counter increment per batch
    idx = arange_idx(16)
    want = ops.prepare_batch_aug(ds.pts, idx, 64, True, True, stages=bits(ops, 'normalize', *FIVE), seed=5, counter=counter_t(0),
                                 **PARAMS)
    assert torch.equal(batches[0][0][..., 0], want)
    # aug=True: today's output, and the same stages spelled as a mapping
    plain, _, _ = _dataset(aug=True, seed=5)
    spelled, _, _ = _dataset(aug={'rotate_z': True, 'jitter': True}, seed=5)
    today = ops.prepare_batch(plain.pts, idx, 64, True, True, seed=5, counter=counter_t(0))
    assert torch.equal(plain.batch(idx)[0][..., 0], today) and torch.equal(spelled.batch(idx)[0][..., 0], today)
    off, _, _ = _dataset(aug={}, seed=5)                        # missing keys: off
    none, _, _ = _dataset(aug=False, seed=5)
    assert torch.equal(off.batch(idx)[0], none.batch(idx)[0])
    with pytest.raises(ValueError, match="'dropout'"):
        UnifiedPointDG('modelnet', pts, labels, pc_input_num=64, aug={'shift': 0.1, 'dropout': 0.5})
    with pytest.raises(RuntimeError, match='scale_low'):
        _dataset(aug={'scale': (1.25, 0.8)})[0].batch(idx)


def _three_steps():
    from bench import BENCH_METHODS
    from sug_amd.data.dataloader import DeviceLoader, UnifiedPointDG
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    g = torch.Generator().manual_seed(21)
    sets = []
    for seed, kind in ((1, 'modelnet'), (2, 'scannet')):
        pts = (torch.rand(24, 1536, 3, generator=g) * 2 - 1).numpy()
        labels = torch.randint(0, 10, (24,), generator=g).numpy()
        sets.append(UnifiedPointDG(kind, pts, labels, pc_input_num=1024, aug=ALL_ON, model='DGCNN', seed=seed))
    src, tgt = (DeviceLoader(s, batch_size=8, shuffle=True, drop_last=True) for s in sets)
    torch.manual_seed(666)
    model = Net_MDA('DGCNN').cuda().train()
    tr = SUGStep(model, lr=1e-3, weight_decay=5e-5, methods=BENCH_METHODS)
    torch.manual_seed(666)
    losses = []
    for (data, label), (data_t, label_t) in zip(src, tgt):
        losses.append([None if v is None else float(v) for v in tr.step(data, label, data_t, label_t)])
    return losses


def test_end_to_end_steps_are_reproducible():
    a = _three_steps()
    b = _three_steps()
    assert len(a) == 3 and all(v is not None and np.isfinite(v) for step in a for v in step)
    assert a == b, 'two runs from the same seeds differ: %r vs %r' % (a, b)


# ------------------------------------------------------------------------------------------------ 11. sharding
def test_rank_sharding(fix):
    from sug_amd.data.dataloader import DeviceLoader, DistributedSampler, build_dataloader
    ds, pts, labels = _dataset(M=10, P=64, N=64)
    full = ds.batch(arange_idx(10))[0]                        # no augmentation: a cloud is identified by its data
    keys = {full[i].cpu().numpy().tobytes(): i for i in range(10)}
    assert len(keys) == 10
    want = fix['sampler_len10']                                 # [shuffle, epoch, rank, 4]
    orders = {}
    for rank in range(A.SAMPLER_WORLD):
        sampler = DistributedSampler(ds, num_replicas=A.SAMPLER_WORLD, rank=rank)
        loader = DeviceLoader(ds, batch_size=2, sampler=sampler)
        assert len(loader) == 2
        for ei, epoch in enumerate(A.SAMPLER_EPOCHS):
            sampler.set_epoch(epoch)
            got = [(keys[d.cpu().numpy().tobytes()], int(l)) for data, label in loader for d, l in zip(data, label)]
            assert [g[0] for g in got] == want[1, ei, rank].tolist(), (rank, epoch)
            assert [g[1] for g in got] == [int(labels[i]) for i in want[1, ei, rank]]
            orders[rank, epoch] = [g[0] for g in got]
    for epoch in A.SAMPLER_EPOCHS:                             # the ranks together: every cloud, two of them twice (12 of 10)
        seen = sum((orders[r, epoch] for r in range(A.SAMPLER_WORLD)), [])
        assert sorted(set(seen)) == list(range(10)) and len(seen) == 12
    assert all(orders[r, 0] != orders[r, 1] for r in range(A.SAMPLER_WORLD)), 'set_epoch must change the order'
    # build_dataloader without a process group: a shuffled loader that drops the last partial batch
    same, loader, sampler = build_dataloader(ds, 4, dist=False, workers=8, seed=3)
    assert same is ds and sampler is None and loader.shuffle and len(loader) == 2
    visited = [keys[d.cpu().numpy().tobytes()] for data, _ in loader for d in data]
    assert len(visited) == 8 and len(set(visited)) == 8
    _, loader, _ = build_dataloader(ds, 4, dist=False, training=False)
    assert not loader.shuffle and [keys[d.cpu().numpy().tobytes()] for data, _ in loader for d in data] == list(range(8))
