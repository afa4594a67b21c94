#!/usr/bin/env python3
"""PointNet++ MSG + feature propagation: forward + backward of the composed network of tests/pn2_msg_fp_cases.py (two
multi-scale set abstractions, a group-all one, three feature propagations; B = 16, N = 2048, npoint 1024 / 256) on the HIP
classes against the torch restatement of the same file on the same GPU, alternated in one process, device events.

    python tools/bench_pn2_seg.py [--iters 50] [--warmup 5] [--out profiles/pn2_msg_fp_bench.json]
    python tools/bench_pn2_seg.py --kernels              # a few launches of each new kernel, for ONE run under
                                                         # `rocprofv3 --kernel-trace --stats` (tools/prof_cmd.sh)
    python tools/bench_pn2_seg.py --merge-stats CSV --out JSON    # per-kernel us and algorithmic bytes / time into the JSON

Algorithmic bytes (each input once, each output once): ball query B(12N + 12S + 4 S sum(ns)) for the multi-radius launch and
sum_r B(12N + 12S + 4 S ns_r) for separate launches; interpolation forward B(24N + 4SD + 4ND + 12N) (idx3, d3, src, out,
w3), backward B(4ND + 24N + 4SD) plus the reverse-list build B(12N + 4(S + 1) + 12N)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

B, N, NP1, NP2 = 16, 2048, 1024, 256
RADII, NSAMPLE = (0.1, 0.2, 0.4), (32, 64, 128)
FP_SHAPES = ((2048, 1024, 128), (1024, 256, 512))          # N, S, D of the last two feature propagations
REPS = 20


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def network(a):
    import pn2_msg_fp_cases as C
    xyz = C.clouds(0, N, batch=B).cuda()
    nets = {}
    for tag, fam in (('hip', C.hip_family()), ('torch', C.Restated)):
        net = C.SegNet(fam, NP1, NP2)
        C.load_seeded(net, 0)
        nets[tag] = net.cuda().train()

    def step(net):
        def f():
            net.zero_grad(set_to_none=True)
            net(xyz).square().mean().backward()
        return f
    steps = {k: step(v) for k, v in nets.items()}
    torch.manual_seed(1)
    y_hip = nets['hip'](xyz).detach()
    torch.manual_seed(1)
    y_t = nets['torch'](xyz).detach()
    for f in steps.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    rounds, per = 5, max(a.iters // 5, 1)
    ms = {'hip': [], 'torch': []}
    for _ in range(rounds):                       # alternated: both see the same clocks and cache state drift
        for k in ('hip', 'torch'):
            ms[k].append(event_ms(steps[k], per))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return {'workload': 'PointNet++ MSG + FP composed network, forward + backward', 'B': B, 'N': N, 'npoint': [NP1, NP2],
            'iters_per_path': rounds * per, 'hip_ms': round(med['hip'], 3), 'torch_restatement_ms': round(med['torch'], 3),
            'hip_ms_rounds': [round(v, 3) for v in ms['hip']], 'torch_ms_rounds': [round(v, 3) for v in ms['torch']],
            'speedup': round(med['torch'] / med['hip'], 2),
            # same parameters and FPS draws; the restatement's distances come from the GPU library GEMM here, so a few pairs at a
            # radius or among the three nearest fall on the other side (the CPU comparison is tests/test_gpu_pn2_msg_fp.py)
            'max_abs_diff_output_vs_gpu_restatement': float((y_hip - y_t).abs().max())}


def kernels():
    """REPS launches of: ball_query_multi (R = 3), three ball_query launches, fp_interp forward and backward at two shapes."""
    import pn2_msg_fp_cases as C
    from sug_amd import ops
    rows = C.clouds(0, N, batch=B).permute(0, 2, 1).contiguous().cuda()
    cen = ops.gather_rows(rows, ops.fps(rows, NP1, torch.zeros(B, dtype=torch.long)))
    for _ in range(REPS):
        ops.ball_query_multi(rows, cen, RADII, NSAMPLE)
    for _ in range(REPS):
        for r, k in zip(RADII, NSAMPLE):
            ops.ball_query(rows, cen, r, k)
    for n, s, d in FP_SHAPES:
        x1 = rows[:, :n].contiguous()
        x2 = ops.gather_rows(x1, ops.fps(x1, s, torch.zeros(B, dtype=torch.long)))
        src = torch.randn(B, s, d, device='cuda', requires_grad=True)
        for _ in range(REPS):
            y = ops.fp_interp(x1, x2, None, src)
            y.backward(torch.ones_like(y))
            src.grad = None
    torch.cuda.synchronize()


def merge_stats(csv_path, out_path):
    import csv
    rows = {r['kernel']: r for r in csv.DictReader(open(csv_path))}

    def total_us(sub):
        hit = [r for k, r in rows.items() if sub in k]
        return sum(float(r['us_per_step']) for r in hit), sum(float(r['calls_per_step']) for r in hit)
    S = NP1
    res = {}
    t, c = total_us('ball_query_multi_kernel')
    by = B * (12 * N + 12 * S + 4 * S * sum(NSAMPLE))
    res['ball_query_multi_R3'] = {'us': round(t / REPS, 2), 'launches': c / REPS, 'algorithmic_MB': round(by / 1e6, 2),
                                  'GB_per_s': round(by / (t / REPS) / 1e3, 1)}
    t, c = total_us('ball_query_lds_kernel')
    by = sum(B * (12 * N + 12 * S + 4 * S * k) for k in NSAMPLE)
    res['ball_query_x3'] = {'us': round(t / REPS, 2), 'launches': c / REPS, 'algorithmic_MB': round(by / 1e6, 2),
                            'GB_per_s': round(by / (t / REPS) / 1e3, 1)}
    # the two interpolation shapes share kernel names: reported as the sum over both shapes, per forward / backward of both
    for name, sub, fn in (('fp_interp_fwd', 'fp_interp_fwd_kernel', lambda n, s, d: B * (24 * n + 4 * s * d + 4 * n * d + 12 * n)),
                          ('fp_interp_bwd', 'fp_interp_bwd_kernel', lambda n, s, d: B * (4 * n * d + 24 * n + 4 * s * d))):
        t, c = total_us(sub)
        by = sum(fn(*sh) for sh in FP_SHAPES)
        res[name] = {'us_both_shapes': round(t / REPS, 2), 'launches': c / REPS, 'algorithmic_MB': round(by / 1e6, 2),
                     'GB_per_s': round(by / (t / REPS) / 1e3, 1), 'shapes_N_S_D': FP_SHAPES}
    cur = json.load(open(out_path)) if os.path.exists(out_path) else {}
    cur['kernels'] = res
    json.dump(cur, open(out_path, 'w'), indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--merge-stats')
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.kernels:
        return kernels()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out)
    res = network(a)
    if a.out:
        cur = json.load(open(a.out)) if os.path.exists(a.out) else {}
        cur.update(res)
        json.dump(cur, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
