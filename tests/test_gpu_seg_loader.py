"""GPU: sug_prepare_seg_batch / ops.prepare_seg_batch / PartSegDataset -- the part-segmentation batch (variable-length clouds,
extra channels, per-point labels) in one launch.

  1. bit for bit against sug_prepare_batch_aug where the two contracts meet (full lengths, no extra channels);
  2. the source indices against the host restatement (tests/seg_loader_cases.py), the labels and the category exactly;
  3. the arithmetic against the fp64 recipe with the reported draws fed back;
  4. a supplied `sel` with repeats; bad sel / idx / lengths entries are marked and their neighbours untouched;
  5. reproducibility and graph capture;
  6. the dataset under DeviceLoader, build_dataloader, seg_eval_worker and SegStep.

Accuracy rule of 3: max-abs deviation <= R * 2^-24, R the fp32 roundings that reach an output coordinate through the enabled
stages (seg_loader_cases.ROUNDINGS, derived in tests/test_gpu_augment.py: coordinates below 2, -ffp-contract=off); all stages
behind normalise and the pre-rotation: R = 34, 2.03e-6; a direction channel passes the three rotations only: R = 24, 1.43e-6.
Measured on an MI355X: DESIGN section 10e."""
import math

import numpy as np
import pytest
import torch

import augment_cases as A
import data_pipeline_cases as C
import seg_cases as S
import seg_loader_cases as SL

pytestmark = pytest.mark.gpu

SEED = SL.SEED
PRE = (1.0, 0.0, 0.0, 0.0, math.cos(-math.pi / 2), -math.sin(-math.pi / 2), 0.0, math.sin(-math.pi / 2), math.cos(-math.pi / 2))
ALL = ('normalize',) + SL.FIVE


def cu(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def counter_t(v=0):
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v], dtype=torch.int64, device='cuda')


def arange_idx(B):
    return torch.arange(B, dtype=torch.int32, device='cuda')


def bits(ops, *stages, normals=False):
    table = {'normalize': ops.PREP_NORMALIZE, 'rotate_z': ops.PREP_ROTATE_Z, 'jitter': ops.PREP_JITTER, 'scale': ops.PREP_SCALE,
             'perturb': ops.PREP_PERTURB, 'shift': ops.PREP_SHIFT}
    return sum(table[s] for s in stages) | (ops.PREP_NORMALS if normals else 0)


_CASES = {}


def case(name, E=3):
    """The host arrays of seg_loader_cases.make_case and their device tensors ('d'); built once per (name, E), read only."""
    if (name, E) not in _CASES:
        c = SL.make_case(name, E)
        c['d'] = {k: (None if c[k] is None else cu(c[k])) for k in ('pts', 'extra', 'point_label', 'category', 'lengths')}
        _CASES[name, E] = c
    return _CASES[name, E]


def seg(c, idx, N, lengths='own', extra='own', **kw):
    from sug_amd import ops
    d = c['d']
    return ops.prepare_seg_batch(d['pts'], d['extra'] if extra == 'own' else extra, d['point_label'], d['category'],
                                 d['lengths'] if isinstance(lengths, str) else lengths, idx, N, **kw)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. against the parent's kernel
@pytest.mark.parametrize('name', ['small', 'big'])
def test_equals_prepare_batch_aug_bit_for_bit(name):
    from sug_amd import ops
    c = case(name)
    B, N = c['M'], c['N']
    kw = dict(stages=bits(ops, *ALL), seed=SEED, counter=counter_t(5), sigma=C.SIGMA, clip=C.CLIP, **SL.PARAMS)
    old = ops.prepare_batch_aug(c['d']['pts'], arange_idx(B), N, True, True, return_draws=True, **kw)
    new = seg(c, arange_idx(B), N, lengths=None, extra=None, pre_matrix=PRE, return_draws=True, **kw)
    assert new[0].shape == (B, 3, N) and torch.equal(new[0], old[0])
    for x, y in zip(old[1:], new[3:]):                          # the six draws
        assert torch.equal(x, y)


def test_equals_prepare_batch_aug_on_the_points_of_a_short_cloud():
    from sug_amd import ops
    B, P, N = 3, 48, 64
    pts = torch.rand(B, P, 3, generator=torch.Generator().manual_seed(3)).cuda()
    lab = torch.zeros(B, P, dtype=torch.uint8, device='cuda')
    cat = torch.zeros(B, dtype=torch.int64, device='cuda')
    kw = dict(stages=bits(ops, *ALL), seed=SEED, counter=counter_t(9), **SL.PARAMS)
    old = ops.prepare_batch_aug(pts, arange_idx(B), N, True, True, **kw)
    new = ops.prepare_seg_batch(pts, None, lab, cat, None, arange_idx(B), N, pre_matrix=PRE, **kw)[0]
    assert torch.equal(new[:, :, :P], old[:, :, :P])
    assert not old[:, :, P:].cpu().numpy().any() and bool(torch.isfinite(new).all()) and bool((new[:, :, P:] != 0).any())


# ------------------------------------------------------------------------------------------------ 2. indices, labels, category
@pytest.mark.parametrize('name', list(SL.CASES))
def test_sources_labels_and_category_are_exact(name):
    from sug_amd import ops
    c = case(name)
    M, P, N = c['M'], c['P'], c['N']
    order = list(range(M))[::-1]                                # slot b holds cloud M-1-b: a slot is not a cloud
    ctr = 5
    points, cat, lab, ang, nz, sel, sc, pn, sh = seg(c, cu(np.array(order, np.int32)), N, stages=bits(ops, *ALL, normals=True),
                                                     seed=SEED, counter=counter_t(ctr), return_draws=True, **SL.PARAMS)
    assert points.shape == (M, 6, N) and points.dtype == torch.float32 and bool(torch.isfinite(points).all())
    assert lab.shape == (M, N) and lab.dtype == torch.int64 and cat.shape == (M,) and cat.dtype == torch.int64
    assert sel.shape == (M, N) and sel.dtype == torch.int32
    sel_h, lab_h = sel.cpu().numpy(), lab.cpu().numpy()
    for b, ci in enumerate(order):
        L = int(c['lengths'][ci])
        want = SL.host_sources(SEED, ctr, b, L, N)
        assert np.array_equal(sel_h[b], want), 'cloud %d (L = %d) in slot %d' % (ci, L, b)
        if L <= N:
            assert sel_h[b, :L].tolist() == list(range(L)) and np.array_equal(sel_h[b, L:], SL.host_fill(SEED, ctr, b, L, N))
        assert np.array_equal(lab_h[b], c['point_label'][ci, sel_h[b]].astype(np.int64))
    assert np.array_equal(cat.cpu().numpy(), c['category'][order])
    # the old draws of the same launch have not moved (tests/test_gpu_augment.py's checks and tolerances)
    assert np.abs(f64(sc) - A.host_scales(SEED, ctr, M)).max() <= 1e-6
    assert np.abs(f64(sh) - A.host_shifts(SEED, ctr, M)).max() <= 1e-6
    assert np.abs(f64(pn) - A.host_perturb_normals(SEED, ctr, M)).max() <= 1e-5
    assert np.abs(f64(ang) - C.host_angles(SEED, ctr, M)).max() <= 1e-6
    assert np.abs(f64(nz) - C.host_normals(SEED, ctr, M, N)).max() <= 1e-5


def test_shuffle_orders_a_short_cloud_by_its_keys():
    from sug_amd import ops
    c = case('small')
    M, N = c['M'], c['N']
    ctr = 3
    _, _, _, _, _, sel, *_ = seg(c, arange_idx(M), N, stages=ops.PREP_NORMALIZE | ops.PREP_SHUFFLE, seed=SEED,
                                 counter=counter_t(ctr), return_draws=True)
    sel = sel.cpu().numpy()
    for b in range(M):
        L = int(c['lengths'][b])
        k = min(L, N)
        assert np.array_equal(sel[b, :k], C.host_subset(SEED, ctr, b + 1, L, k)[b])
        assert np.array_equal(sel[b, k:], SL.host_fill(SEED, ctr, b, L, N))


# ------------------------------------------------------------------------------------------------ 3. arithmetic
@pytest.mark.parametrize('name, stages, pre', [('small', ALL, True), ('mid', ALL, True), ('big', ALL, True),
                                               ('small', ('normalize',), False), ('small', ('normalize', 'rotate_z', 'scale'), False)])
def test_arithmetic_against_the_fp64_recipe(name, stages, pre):
    from sug_amd import ops
    c = case(name)
    M, N = c['M'], c['N']
    points, _, _, ang, nz, sel, sc, pn, sh = seg(c, arange_idx(M), N, stages=bits(ops, *stages, normals=True), seed=SEED,
                                                 counter=counter_t(11), pre_matrix=PRE if pre else None, sigma=C.SIGMA, clip=C.CLIP,
                                                 return_draws=True, **SL.PARAMS)
    got = f64(points)
    ang, nz, sel, sc, pn, sh = ang.cpu().numpy(), nz.cpu().numpy(), sel.cpu().numpy(), sc.cpu().numpy(), pn.cpu().numpy(), sh.cpu().numpy()
    enabled = tuple(stages) + (('pre',) if pre else ())
    lim_xyz = SL.bound(enabled)
    lim_dir = SL.bound([s for s in enabled if s in SL.NORMAL_STAGES])
    dev_xyz = dev_dir = dev_len = 0.0
    for b in range(M):
        want = SL.recipe(c['pts'][b], c['extra'][b], int(c['lengths'][b]), sel[b], stages, pre=PRE if pre else None, angle=ang[b],
                         noise=nz[b], scale=sc[b], normals=pn[b], shift=sh[b], turn=True)
        dev_xyz = max(dev_xyz, np.abs(got[b, :3] - want[:3]).max())
        dev_dir = max(dev_dir, np.abs(got[b, 3:] - want[3:]).max())
        dev_len = max(dev_len, np.abs(np.sqrt((got[b, 3:] ** 2).sum(axis=0)) - 1.0).max())
    print('%s %s: xyz dev %.3e (bound %.3e), direction dev %.3e, | |n| - 1 | %.3e (bound %.3e)'
          % (name, '+'.join(enabled), dev_xyz, lim_xyz, dev_dir, dev_len, lim_dir))
    assert dev_xyz <= lim_xyz
    if lim_dir == 0.0:                                          # no rotation: the direction is the gathered input
        assert dev_dir == 0.0
    assert dev_dir <= lim_dir and dev_len <= max(lim_dir, 3 * 2.0 ** -24)   # the fp32 input direction itself: 3 roundings off unit length


@pytest.mark.parametrize('normals', [False, True])
def test_extra_channels_are_copied_through(normals):
    from sug_amd import ops
    c = case('small', 5)
    M, N = c['M'], c['N']
    points, _, _, _, _, sel, *_ = seg(c, arange_idx(M), N, stages=bits(ops, *ALL, normals=normals), seed=SEED, counter=counter_t(2),
                                      pre_matrix=PRE, return_draws=True, **SL.PARAMS)
    assert points.shape == (M, 8, N)
    gathered = torch.gather(c['d']['extra'], 1, sel.long().unsqueeze(-1).expand(-1, -1, 5)).transpose(1, 2)     # [M, 5, N]
    if normals:
        assert torch.equal(points[:, 6:], gathered[:, 3:])
        assert not torch.equal(points[:, 3:6], gathered[:, :3]), 'the direction did not turn'
    else:
        assert torch.equal(points[:, 3:], gathered)


# ------------------------------------------------------------------------------------------------ 4. supplied sel, bad inputs
def _sel_case():
    """'small' with N = 128 > P = 96: base [M, P] takes point n % L, rep [M, 128] random points of each cloud, with repeats."""
    c = case('small')
    M, P = c['M'], c['P']
    r = np.random.RandomState(4)
    L = c['lengths'].astype(np.int64)[:, None]
    base = (np.arange(P)[None, :] % L).astype(np.int32)
    rep = (r.randint(0, 1 << 30, size=(M, 128)) % L).astype(np.int32)
    rep[:, 1] = rep[:, 0]                                       # a repeat in every cloud, also where L is large
    return c, base, rep


def test_supplied_sel_with_repeats_is_followed_exactly():
    from sug_amd import ops
    c, base, rep = _sel_case()
    M, P = c['M'], c['P']
    # per-cloud draws only (no jitter): an output row is a function of its source point
    kw = dict(stages=bits(ops, 'normalize', 'rotate_z', 'scale', 'perturb', 'shift', normals=True), seed=SEED, counter=counter_t(6),
              pre_matrix=PRE, **SL.PARAMS)
    ref, cat0, lab0 = seg(c, arange_idx(M), P, sel=cu(base), **kw)
    out, cat, lab, _, _, sel_out, *_ = seg(c, arange_idx(M), 128, sel=cu(rep), return_draws=True, **kw)
    assert torch.equal(sel_out, cu(rep)) and torch.equal(cat, cat0) and bool(torch.isfinite(out).all())
    take = cu(rep).long()
    assert torch.equal(out, torch.gather(ref, 2, take.unsqueeze(1).expand(-1, 6, -1)))
    assert torch.equal(lab, torch.gather(lab0, 1, take))
    assert np.array_equal(lab.cpu().numpy(), np.take_along_axis(c['point_label'].astype(np.int64), rep.astype(np.int64), axis=1))
    # supplied sel and supplied draws: no counter is needed
    only = seg(c, arange_idx(M), 128, sel=cu(rep), stages=ops.PREP_NORMALIZE)
    assert bool(torch.isfinite(only[0]).all()) and torch.equal(only[2], lab)


def _assert_marked(got, clean, bad_rows=(), bad_clouds=()):
    """got / clean: (points, category, label).  The listed (cloud, row) pairs and clouds are NaN with label -1 (a cloud:
    category -1 too); everything else equals the clean call bit for bit."""
    pts, cat, lab = (t.clone() for t in got)
    for b, n in bad_rows:
        assert bool(torch.isnan(pts[b, :, n]).all()) and int(lab[b, n]) == -1
        pts[b, :, n], lab[b, n] = clean[0][b, :, n], clean[2][b, n]
    for b in bad_clouds:
        assert bool(torch.isnan(pts[b]).all()) and bool((lab[b] == -1).all()) and int(cat[b]) == -1
        pts[b], lab[b], cat[b] = clean[0][b], clean[2][b], clean[1][b]
    assert bool(torch.isfinite(clean[0]).all())
    assert torch.equal(pts, clean[0]) and torch.equal(cat, clean[1]) and torch.equal(lab, clean[2])


def test_bad_sel_entries_mark_their_row_only():
    from sug_amd import ops
    c, _, rep = _sel_case()
    M = c['M']
    kw = dict(stages=bits(ops, *ALL, normals=True), seed=SEED, counter=counter_t(6), pre_matrix=PRE, **SL.PARAMS)
    clean = seg(c, arange_idx(M), 128, sel=cu(rep), **kw)
    bad = rep.copy()
    bad[1, 5] = c['lengths'][1]                                 # L itself: 70 of P = 96, a row of the resident array but not of the cloud
    bad[3, 0] = -1
    bad[4, 127] = 2 ** 31 - 1
    _assert_marked(seg(c, arange_idx(M), 128, sel=cu(bad), **kw), clean, bad_rows=[(1, 5), (3, 0), (4, 127)])


def test_bad_idx_entries_mark_their_cloud_only():
    from sug_amd import ops
    c = case('small')
    M, N = c['M'], c['N']
    kw = dict(stages=bits(ops, *ALL, normals=True), seed=SEED, counter=counter_t(8), **SL.PARAMS)
    clean = seg(c, arange_idx(M), N, **kw)
    idx = torch.tensor([0, -1, 2, M, 4], dtype=torch.int32, device='cuda')
    got = seg(c, idx, N, return_draws=True, **kw)
    _assert_marked(got[:3], clean, bad_clouds=[1, 3])
    assert bool((got[5][[1, 3]] == -1).all()), 'sel_out of a cloud that was not read'


def test_bad_lengths_mark_their_cloud_only():
    from sug_amd import ops
    c = case('small')
    M, P, N = c['M'], c['P'], c['N']
    kw = dict(stages=bits(ops, *ALL, normals=True), seed=SEED, counter=counter_t(8), **SL.PARAMS)
    clean = seg(c, arange_idx(M), N, **kw)
    lengths = c['lengths'].copy()
    lengths[1], lengths[3] = 0, P + 1
    _assert_marked(seg(c, arange_idx(M), N, lengths=cu(lengths), **kw), clean, bad_clouds=[1, 3])
    lengths[1], lengths[3] = -5, 2 ** 31 - 1
    _assert_marked(seg(c, arange_idx(M), N, lengths=cu(lengths), **kw), clean, bad_clouds=[1, 3])


def test_marked_labels_fail_loudly_downstream():
    """A label of -1 is not ignore_index: the loss is NaN and the IoU books raise their error word."""
    from sug_amd import ops
    lab = torch.zeros(2, 8, dtype=torch.int64, device='cuda')
    lab[1, 3] = -1
    z = torch.zeros(2, 8, 6, device='cuda')
    assert bool(torch.isnan(ops.point_ce(z, lab)))
    state = ops.part_iou_state('cuda')
    ops.part_iou_accumulate(z, lab, torch.zeros(2, dtype=torch.int64, device='cuda'), S.PART_FIRST, S.PART_COUNT, state)
    assert ops.part_iou_state_fields(state)['error'] == 1


# ------------------------------------------------------------------------------------------------ 5. reproducibility, capture
def test_reproducible_from_seed_and_counter():
    from sug_amd import ops
    c = case('small')
    N = c['N']
    idx = torch.tensor([0, 0, 3, 3, 1], dtype=torch.int32, device='cuda')       # cloud 0 (a subset) and cloud 3 (a fill) twice
    run = lambda ctr, seed=SEED: seg(c, idx, N, stages=bits(ops, *ALL, normals=True), seed=seed, counter=counter_t(ctr),
                                     return_draws=True, **SL.PARAMS)
    a, b, nxt, other = run(41), run(41), run(42), run(41, SEED + 1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for r in (nxt, other):
        assert not torch.equal(a[0], r[0]) and not torch.equal(a[5], r[5]) and torch.equal(a[1], r[1])
    sel = a[5].cpu().numpy()
    assert not np.array_equal(sel[0], sel[1]), 'the same cloud twice in a batch: the same subset'
    assert np.array_equal(sel[2, :41], sel[3, :41]) and not np.array_equal(sel[2, 41:], sel[3, 41:]), 'the same fill'
    assert not torch.equal(a[0][0], a[0][1])
    # a cloud's output depends on the batch through its slot only
    alone = seg(c, idx[:3].contiguous(), N, stages=bits(ops, *ALL, normals=True), seed=SEED, counter=counter_t(41), **SL.PARAMS)
    assert torch.equal(alone[0], a[0][:3]) and torch.equal(alone[2], a[2][:3])


def test_graph_capture_replays_with_fresh_draws():
    from sug_amd import ops
    c = case('small')
    M, N, B = c['M'], c['N'], 4
    idx = arange_idx(B)
    cnt = counter_t(100)
    out = torch.empty(B, 6, N, device='cuda')
    lab = torch.empty(B, N, dtype=torch.int64, device='cuda')
    cat = torch.empty(B, dtype=torch.int64, device='cuda')
    kw = dict(stages=bits(ops, *ALL, normals=True), seed=SEED, pre_matrix=PRE, **SL.PARAMS)
    seg(c, idx, N, counter=cnt, out=out, label_out=lab, category_out=cat, **kw)            # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seg(c, idx, N, counter=cnt, out=out, label_out=lab, category_out=cat, **kw)
    seen = []
    for r in range(3):
        idx.copy_(torch.tensor([(r + 2 * i) % M for i in range(B)], dtype=torch.int32))
        cnt.add_(1)
        graph.replay()
        eager = seg(c, idx.clone(), N, counter=cnt.clone(), **kw)
        assert torch.equal(out, eager[0]) and torch.equal(cat, eager[1]) and torch.equal(lab, eager[2]), 'replay %d' % r
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])


# ------------------------------------------------------------------------------------------------ 6. dataset and loader
PART_FIRST, PART_COUNT = [0, 3, 5], [3, 2, 3]                   # three categories over the model case's eight parts


def _dataset(lengths, N, seed=0, aug=True, packed=False):
    """Ragged clouds [L_m, 6] (xyz in the unit cube, unit normals) with labels inside each category's range."""
    from sug_amd.data import PartSegDataset, pack_clouds
    r = np.random.RandomState(17)
    clouds, labels = [], []
    cat = np.arange(len(lengths)) % 3
    for L, k in zip(lengths, cat):
        v = r.randn(L, 3)
        clouds.append(np.concatenate([r.uniform(-0.5, 0.5, (L, 3)), v / np.linalg.norm(v, axis=1, keepdims=True)], axis=1).astype(np.float32))
        labels.append(PART_FIRST[k] + r.randint(0, PART_COUNT[k], L))
    if packed:                                                  # the array form: [M, P, 6] with explicit lengths
        pts, own = pack_clouds(clouds)
        ds = PartSegDataset(pts, pack_clouds(labels)[0], cat, PART_FIRST, PART_COUNT, lengths=own, num_points=N, aug=aug, seed=seed)
    else:
        ds = PartSegDataset(clouds, labels, cat, PART_FIRST, PART_COUNT, num_points=N, aug=aug, seed=seed)
    return ds, clouds, labels, cat


def test_loader_batches_in_segstep_order():
    from sug_amd import ops
    from sug_amd.data.dataloader import DeviceLoader
    lengths, N = (30, 80, 64, 100, 12, 65, 50), 64
    ds, clouds, labels, cat = _dataset(lengths, N, seed=5)
    assert len(ds) == 7 and ds.seed == 5 and ds.device.type == 'cuda' and ds.extra_channels == 3
    assert ds.stages == ops.PREP_NORMALIZE | ops.PREP_SCALE | ops.PREP_SHIFT | ops.PREP_NORMALS
    batches = list(DeviceLoader(ds, batch_size=3))
    assert [len(b) for b in batches] == [3, 3, 3]
    assert [tuple(b[0].shape) for b in batches] == [(3, 6, N), (3, 6, N), (1, 6, N)]
    assert [tuple(b[1].shape) for b in batches] == [(3,), (3,), (1,)] and [tuple(b[2].shape) for b in batches] == [(3, N), (3, N), (1, N)]
    assert all(p.dtype == torch.float32 and k.dtype == torch.int64 and l.dtype == torch.int64 and p.is_cuda and k.is_cuda and l.is_cuda
               for p, k, l in batches)
    assert int(ds.counter) == 3                                 # one counter increment per batch
    for k, (points, category, label) in enumerate(batches):
        ids = list(range(3 * k, min(3 * k + 3, 7)))
        eager = ops.prepare_seg_batch(ds.pts, ds.extra, ds.point_labels, ds.categories, ds.lengths, cu(np.array(ids, np.int32)), N,
                                      stages=ds.stages, seed=5, counter=counter_t(k), return_draws=True, **ds.aug_kw)
        assert torch.equal(points, eager[0]) and torch.equal(category, eager[1]) and torch.equal(label, eager[2])
        sel = eager[5].cpu().numpy()
        assert category.cpu().tolist() == [int(cat[i]) for i in ids]
        for b, i in enumerate(ids):
            assert np.array_equal(sel[b], SL.host_sources(5, k, b, lengths[i], N))
            assert np.array_equal(label[b].cpu().numpy(), labels[i][sel[b]])
    # the packed-array form of the same data is the same dataset
    same, *_ = _dataset(lengths, N, seed=5, packed=True)
    again = same.batch([0, 1, 2])
    assert all(torch.equal(x, y) for x, y in zip(again, batches[0]))


def test_getitem_and_build_dataloader():
    from sug_amd.data.dataloader import DeviceLoader, build_dataloader
    lengths, N = (30, 80, 64, 100, 12, 65, 50), 64
    ds, *_ = _dataset(lengths, N, seed=9)
    other, *_ = _dataset(lengths, N, seed=9)
    for i in (3, 4):                                            # both datasets stand at the same counter
        item, (points, category, label) = ds[i], other.batch([i])
        assert item[0].shape == (6, N) and item[2].shape == (N,)
        assert torch.equal(item[0], points[0]) and torch.equal(item[1], category[0]) and torch.equal(item[2], label[0])
    assert int(ds.counter) == 2
    same, loader, sampler = build_dataloader(ds, 2, dist=False)
    assert same is ds and sampler is None and isinstance(loader, DeviceLoader) and len(loader) == 3
    got = list(loader)
    assert len(got) == 3 and all(len(b) == 3 and b[0].shape == (2, 6, N) and b[1].shape == (2,) and b[2].shape == (2, N) for b in got)
    out = (torch.empty(2, 6, N, device='cuda'), torch.empty(2, dtype=torch.int64, device='cuda'),
           torch.empty(2, N, dtype=torch.int64, device='cuda'))
    assert all(x is y for x, y in zip(ds.batch([0, 1], out=out), out))
    assert out[1].cpu().tolist() == [0, 1] and bool(torch.isfinite(out[0]).all()) and int(out[2].min()) >= 0


def _model():
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    m = S.MODEL
    torch.manual_seed(4)
    return Pointnet2PartSeg(num_part=m['num_part'], num_category=m['num_category'], extra_channels=3, npoint1=m['npoint1'],
                            npoint2=m['npoint2']).cuda()


def test_end_to_end_eval():
    from sug_amd.data.dataloader import DeviceLoader
    from sug_amd.utils.seg_utils import seg_eval_worker
    N = S.MODEL['N']
    ds, *_ = _dataset((100, 160, 220, 280, 340, 400), N, aug=False)
    out = seg_eval_worker(_model(), DeviceLoader(ds, batch_size=3), ds.meter())        # an IndexError here: a cloud was not scored
    assert out['shapes'] == 6 and out['rows'] == 6 * N
    assert np.isfinite(out['loss']) and 0.0 <= out['instance_miou'] <= 1.0
    assert out['category_shapes'].tolist() == [2, 2, 2]


def test_end_to_end_training():
    from sug_amd.data.dataloader import DeviceLoader
    from sug_amd.seg_step import SegStep
    N, B = S.MODEL['N'], 3
    ds, *_ = _dataset((100, 160, 220, 280, 340, 400), N, aug=True, seed=2)
    step = SegStep(_model().train(), lr=1e-3)
    losses = [step.step(*batch) for batch in DeviceLoader(ds, batch_size=B, shuffle=True)]
    assert len(losses) == 2 and all(np.isfinite(float(v)) for v in losses)
    assert step.epoch_totals()[1] == 2 * B * N
