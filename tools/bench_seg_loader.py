#!/usr/bin/env python3
"""What the part-segmentation loader costs: M = 4096 resident clouds of up to P = 4096 points (lengths uniform in
[1024, 4096]), three extra channels (normals), N = 2048, batch 16, aug=True (normalise, random scale, random shift).  Device
events around back-to-back work, the variants alternated window by window in one process, medians and the window-to-window
spread (max - min) of each:

(a) sug_prepare_seg_batch alone: one launch writes points [16, 6, 2048], labels and categories;
(b) sug_prepare_batch_aug at the same P, N and batch with full lengths and no extra channels: the yardstick for what the
    extra channels, the labels and the per-cloud lengths cost;
(c) the same batch composed from torch operations on the same GPU (written here, never used by the product);
(d) one SegStep of Pointnet2PartSeg fed by DeviceLoader(PartSegDataset) against the same step on one resident batch.

    python tools/bench_seg_loader.py [--out profiles/seg_loader_bench.json]

Nothing is gated: every number is written to the JSON."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, P, N, B, E = 4096, 4096, 2048, 16, 3
PART_COUNT = [3] * 14 + [4, 4]                                  # 16 categories over 50 parts, as ShapeNet-Part
PART_FIRST = np.concatenate([[0], np.cumsum(PART_COUNT)[:-1]]).tolist()
SCALE, SHIFT = (0.8, 1.25), 0.1


def torch_batch(pts, extra, labels, categories, lengths, idx, gen):
    """The batch of sug_prepare_seg_batch composed from torch operations, batched over the clouds (no host loop, no host
    wait): normalise over the valid points, an ordered random subset of a long cloud, a short one followed by draws with
    replacement, random scale and shift, the gathers and the transpose."""
    dev = pts.device
    L = lengths[idx].long()
    x = pts[idx]
    ar = torch.arange(P, device=dev)
    valid = (ar[None, :] < L[:, None])
    w = valid.unsqueeze(-1).to(x.dtype)
    mean = (x.double() * w).sum(dim=1, keepdim=True) / L.view(-1, 1, 1)
    x = ((x.double() - mean).float()) * w
    x = x / x.square().sum(dim=2).max(dim=1).values.sqrt().view(-1, 1, 1)
    keys = torch.rand(len(idx), P, device=dev, generator=gen).masked_fill(~valid, 2.0)
    subset = keys.argsort(dim=1)[:, :N]
    fill = (torch.rand(len(idx), N, device=dev, generator=gen) * L[:, None]).long().clamp_(max=P - 1)
    rows = ar[:N][None, :]
    src = torch.where(L[:, None] > N, subset, torch.where(rows < L[:, None], rows.expand(len(idx), -1), fill))
    x = torch.gather(x, 1, src.unsqueeze(-1).expand(-1, -1, 3))
    x = x * (SCALE[0] + torch.rand(len(idx), 1, 1, device=dev, generator=gen) * (SCALE[1] - SCALE[0]))
    x = x + (2 * torch.rand(len(idx), 1, 3, device=dev, generator=gen) - 1) * SHIFT
    e = torch.gather(extra[idx], 1, src.unsqueeze(-1).expand(-1, -1, E))
    points = torch.cat([x, e], dim=2).transpose(1, 2).contiguous()
    return points, categories[idx], torch.gather(labels[idx], 1, src).long()


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / count                   # microseconds per call


def alternate(run, counts, windows):
    """{name: [us per call, one entry per window]}: the variants take turns, so each sees the same machine state."""
    out = {k: [] for k in run}
    for _ in range(windows):
        for k, f in run.items():
            out[k].append(timed(f, counts[k]))
    return out


def summary(w):
    return {k: {'median_us': sorted(v)[len(v) // 2], 'spread_us': max(v) - min(v), 'windows_us': v} for k, v in w.items()}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=5000, help='(a) and (b): launches per window')
    ap.add_argument('--torch-batches', type=int, default=200, help='(c): batches per window')
    ap.add_argument('--steps', type=int, default=40, help='(d): steps per window (about half a second)')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seg_loader_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('bench_seg_loader needs a HIP device; there is no CPU path')
    from sug_amd import _lib, ops
    from sug_amd.data import PartSegDataset
    from sug_amd.data.dataloader import DeviceLoader
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    from sug_amd.seg_step import SegStep

    dev = torch.device('cuda:0')
    r = np.random.RandomState(0)
    cloud = r.uniform(-1.0, 1.0, size=(M, P, 3)).astype(np.float32) + r.uniform(-0.5, 0.5, size=(M, 1, 3)).astype(np.float32)
    nrm = r.standard_normal(size=(M, P, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    lengths = r.randint(1024, P + 1, size=M).astype(np.int32)
    cat = r.randint(0, len(PART_COUNT), size=M)
    lab = (np.asarray(PART_FIRST)[cat][:, None] + r.randint(0, 3, size=(M, P))).astype(np.uint8)
    ds = PartSegDataset(np.concatenate([cloud, nrm], axis=2), lab, cat, PART_FIRST, PART_COUNT, lengths=lengths, num_points=N,
                        aug=True, seed=1, device=dev)
    del cloud, nrm

    # (a), (b), (c): one batch of 16 clouds
    L = _lib.lib()
    p, st = ops._p, ops._st
    idx = torch.as_tensor(r.permutation(M)[:B].astype(np.int32)).to(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    out_a = torch.empty(B, 3 + E, N, device=dev)
    lab_a = torch.empty(B, N, dtype=torch.int64, device=dev)
    cat_a = torch.empty(B, dtype=torch.int64, device=dev)
    out_b = torch.empty(B, 3, N, device=dev)
    params = (ctypes.c_float * ops.PREP_AUG_PARAMS)()
    for slot, v in zip(ops._PREP_AUG_SLOTS, (SCALE[0], SCALE[1], SHIFT, 0.06, 0.18)):
        params[slot] = v
    stages_b = ops.PREP_NORMALIZE | ops.PREP_SCALE | ops.PREP_SHIFT
    assert ds.stages == stages_b | ops.PREP_NORMALS
    gen = torch.Generator(device=dev).manual_seed(0)
    run = {
        'a_prepare_seg_batch': lambda: L.sug_prepare_seg_batch(
            p(ds.pts), p(ds.extra), p(ds.point_labels), p(ds.categories), p(ds.lengths), M, P, E, p(idx), B, N, ds.stages, None,
            None, None, None, None, None, None, 1, p(counter), 0.01, 0.05, params, p(out_a), p(lab_a), p(cat_a), None, None, None,
            None, None, None, st()),
        'b_prepare_batch_aug_full_lengths_no_extra': lambda: L.sug_prepare_batch_aug(
            p(ds.pts), M, P, p(idx), B, N, stages_b, None, None, None, None, None, None, None, 1, p(counter), 0.01, 0.05, params,
            p(out_b), None, None, None, None, None, None, st()),
        'c_torch_composed': lambda: torch_batch(ds.pts, ds.extra, ds.point_labels, ds.categories, ds.lengths, idx.long(), gen),
    }
    for k in ('a_prepare_seg_batch', 'b_prepare_batch_aug_full_lengths_no_extra'):
        for _ in range(200):
            if run[k]() != 0:
                raise RuntimeError('%s failed: %s' % (k, L.sug_last_error()))
    for _ in range(10):
        got = run['c_torch_composed']()
    torch.cuda.synchronize()
    assert got[0].shape == out_a.shape and got[2].shape == lab_a.shape and torch.equal(got[1], cat_a)
    assert bool(torch.isfinite(out_a).all()) and int(lab_a.min()) >= 0
    kernels = alternate(run, {'a_prepare_seg_batch': a.launches, 'b_prepare_batch_aug_full_lengths_no_extra': a.launches,
                              'c_torch_composed': a.torch_batches}, a.windows)

    # (d): the training step, fed by the loader against one resident batch
    torch.manual_seed(0)
    model = Pointnet2PartSeg(num_part=sum(PART_COUNT), num_category=len(PART_COUNT), extra_channels=E).to(dev).train()
    step = SegStep(model, lr=1e-3)
    loader = DeviceLoader(ds, batch_size=B, shuffle=True, drop_last=True)

    def epochs():
        while True:
            yield from loader

    feed = epochs()
    resident = tuple(t.clone() for t in next(feed))

    def loader_step():
        step.step(*next(feed))

    steps = {'d_step_fed_by_loader': loader_step, 'd_step_on_resident_batch': lambda: step.step(*resident)}
    for f in steps.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    step_windows = alternate(steps, {k: a.steps for k in steps}, a.windows)

    s, d = summary(kernels), summary(step_windows)
    result = {'device': torch.cuda.get_device_name(0),
              'shape': {'M': M, 'P': P, 'N': N, 'batch': B, 'extra_channels': E, 'lengths': 'uniform in [1024, 4096]',
                        'stages': 'normalise, scale (0.8, 1.25), shift 0.1, normals'},
              'per_window': {'launches': a.launches, 'torch_batches': a.torch_batches, 'steps': a.steps, 'windows': a.windows},
              'kernel_us_back_to_back': s, 'step_us': d,
              'a_minus_b_us': s['a_prepare_seg_batch']['median_us'] - s['b_prepare_batch_aug_full_lengths_no_extra']['median_us'],
              'c_over_a': s['c_torch_composed']['median_us'] / s['a_prepare_seg_batch']['median_us'],
              'loader_minus_resident_step_us': d['d_step_fed_by_loader']['median_us'] - d['d_step_on_resident_batch']['median_us'],
              'step_loss_totals': step.epoch_totals()[:2]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
