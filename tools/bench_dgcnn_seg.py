#!/usr/bin/env python3
"""DGCNN part segmentation: the fused two-layer EdgeConv block against its composed form IN THE SAME TREE (SUG_EDGE2_FUSED=0's
path: every k-expanded tensor stored), on the same GPU, alternated in one process, device events, the median of 5 rounds
with every round reported (the spread is max - min of the rounds).

  block     one 64 -> 64 block forward + backward at B = 32, N = 1024, k = 20 from [P | Q] and the lists
  seg_step  one SegStep(DGCNNPartSeg) at B = 32, N = 1024, fused | composed, with launch counts
  pn2_step  for context: one SegStep(Pointnet2PartSeg) on the same batch

    python tools/bench_dgcnn_seg.py [--iters 25] [--warmup 3] [--out profiles/dgcnn_seg_bench.json]
    python tools/bench_dgcnn_seg.py --npoints 2048 --out profiles/dgcnn_seg_bench.json

--npoints N (other than 1024) measures seg_step alone at B = 32 * 1024 / N clouds of N points, the same edge count, and adds
it to the file as `seg_step_n<N>` beside the rows that are there.  At N = 2048 the backward's reverse lists (40 960 entries
per cloud) come from the tiled build behind sug_knn_reverse.

Launches are counted with torch.profiler over one call of each path (kernel events; null where the profiler is unavailable).
Edge-sized traffic of the block, counted from the code (nobody measured it): one edge-sized tensor = B N k 64 floats =
168 MB; fused forward writes y1 and a1 and reads y1 once (3), composed forward writes the gathered rows, y1, a1, y2, a2 and
reads each of them once or twice (about 11)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# 32 clouds of 1024 points: the edge count of 16 x 2048 (655 360 rows), the size --npoints 2048 measures.
B, N, K, C1 = 32, 1024, 20, 64
PARTS, CATS = 50, 16
ROUNDS = 5


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def launches(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception:       # noqa: BLE001 -- a count is a side note of the timing
        return None


def alternate(paths, a):
    for f in paths.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    per = max(a.iters // ROUNDS, 1)
    ms = {k: [] for k in paths}
    for _ in range(ROUNDS):                       # alternated: the paths see the same clocks and cache state drift
        for k, f in paths.items():
            ms[k].append(event_ms(f, per))
    out = {'iters_per_path': ROUNDS * per}
    for k, v in ms.items():
        out[k + '_ms'] = round(sorted(v)[len(v) // 2], 3)
        out[k + '_ms_rounds'] = [round(x, 3) for x in v]
        out[k + '_ms_spread'] = round(max(v) - min(v), 3)
        out[k + '_launches'] = launches(paths[k])
    return out


def with_fused(flag, fn):
    from sug_amd import ops

    def run():
        keep, ops.EDGE2_FUSED = ops.EDGE2_FUSED, flag
        try:
            fn()
        finally:
            ops.EDGE2_FUSED = keep
    return run


def bench_block(a):
    from sug_amd import ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, N, C1, generator=g).cuda()
    pq = torch.randn(B, N, 2 * C1, generator=g).cuda().requires_grad_(True)
    idx = ops.knn(x, K)
    W = (torch.randn(C1, C1, generator=g) / 8).cuda().requires_grad_(True)
    bn1, bn2 = torch.nn.BatchNorm2d(C1).cuda().train(), torch.nn.BatchNorm2d(C1).cuda().train()
    gout = torch.randn(B, N, C1, generator=g).cuda()
    params = [pq, W, bn1.weight, bn1.bias, bn2.weight, bn2.bias]

    def block():
        out = ops.edgeconv2(pq, idx, bn1, 0.2, W, None, bn2, 0.2)
        torch.autograd.grad(out, params, gout)
    res = alternate({'fused': with_fused(True, block), 'composed': with_fused(False, block)}, a)
    res.update(B=B, N=N, k=K, C1=C1, Co=C1, edge_tensor_MB=round(B * N * K * C1 * 4 / 1e6, 1),
               speedup=round(res['composed_ms'] / res['fused_ms'], 3))
    return res


def _batch(B=B, N=N):
    import pn2_msg_fp_cases as PC
    pts = PC.clouds(0, N, batch=B).cuda()
    g = torch.Generator().manual_seed(2)
    cat = torch.randint(0, CATS, (B,), generator=g).cuda()
    lab = torch.randint(0, PARTS, (B, N), generator=g).cuda()
    return pts, cat, lab


def bench_step(a, B=B, N=N):
    from sug_amd.model.dgcnn_seg import DGCNNPartSeg
    from sug_amd.seg_step import SegStep
    pts, cat, lab = _batch(B, N)
    steps = []
    for _ in range(2):
        torch.manual_seed(0)
        steps.append(SegStep(DGCNNPartSeg(num_part=PARTS, num_category=CATS).cuda().train()))
    res = alternate({'fused': with_fused(True, lambda: steps[0].step(pts, cat, lab)),
                     'composed': with_fused(False, lambda: steps[1].step(pts, cat, lab))}, a)
    res.update(B=B, N=N, k=K, speedup=round(res['composed_ms'] / res['fused_ms'], 3))
    return res


def bench_pn2(a):
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    from sug_amd.seg_step import SegStep
    pts, cat, lab = _batch()
    torch.manual_seed(0)
    step = SegStep(Pointnet2PartSeg(num_part=PARTS, num_category=CATS).cuda().train())
    res = alternate({'pointnet2': lambda: step.step(pts, cat, lab)}, a)
    res.update(B=B, N=N)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--npoints', type=int, default=N)
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.npoints != N:
        if a.npoints < K or (B * N) % a.npoints:
            ap.error('--npoints must divide %d and be at least k = %d' % (B * N, K))
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res['seg_step_n%d' % a.npoints] = bench_step(a, B * N // a.npoints, a.npoints)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, 'w'), indent=1)
        print(json.dumps(res['seg_step_n%d' % a.npoints]))
        return
    res = {'workload': 'DGCNN part segmentation: two-layer EdgeConv block and SegStep, fused vs composed, same tree',
           'block': bench_block(a), 'seg_step': bench_step(a), 'pn2_step': bench_pn2(a)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
