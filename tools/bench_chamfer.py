#!/usr/bin/env python3
"""Forward + backward of mmd.cd_distance(batch_loss=False) through the ChamferDistance op, on one GPU.  Prints one JSON line.

The parent commit cannot run the op, so the baseline is the COMPOSED form on the same GPU and tree: the [B,N,M,3] difference
tensor, its squared sum, `min` in both directions, the two means, then autograd (torch ops only).  Shapes B x N x M: 64 x 1024 x 1024 and 32 x 2048 x 2048, uniform(-1, 1) clouds, seeded.
Method: both forms in ONE process, alternating: `--rounds` rounds after one that is not kept, in each the composed form's
window, then the op's; a window is at least `--window` seconds of calls (sized from a short probe after the warm-up) and
ends in a device synchronise; profiler off.  Per form: median ms per call over all windows and the spread (max - min) / median between them.
Launches and kernel times come from a pass of their own under torch.profiler (3 calls, device events only): launches per
call of both forms, the microseconds of the op's two kernels, and -- for orientation -- of the two chamfer_dir_kernel
launches of ops.chamfer (sug_chamfer, the detached scalar) at the same shape.

Usage: python tools/bench_chamfer.py [--rounds 4] [--window 0.3] [--out profiles/chamfer_nn_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SHAPES = ((64, 1024, 1024), (32, 2048, 2048))
WARMUP = 3


def _callers(B, N, M):
    import torch
    from sug_amd import ops
    from sug_amd.chamfer_distance import ChamferDistance
    from sug_amd.model import mmd
    g = torch.Generator().manual_seed(B + N)
    x1 = (torch.rand(B, N, 3, generator=g) * 2 - 1).cuda().requires_grad_(True)
    x2 = (torch.rand(B, M, 3, generator=g) * 2 - 1).cuda().requires_grad_(True)
    cd = ChamferDistance()

    def op():
        x1.grad = x2.grad = None
        mmd.cd_distance(x1, x2, cd, batch_loss=False).backward()
        return x1.grad, x2.grad

    def composed():
        x1.grad = x2.grad = None
        d = ((x1[:, :, None, :] - x2[:, None, :, :]) ** 2).sum(-1)
        (d.min(dim=2)[0].mean() + d.min(dim=1)[0].mean()).backward()
        return x1.grad, x2.grad

    def scalar():
        return ops.chamfer(x1, x2)
    return {'composed': composed, 'op': op, 'sug_chamfer': scalar}


def _window(call, k):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(k):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / k * 1e3


def _profile(call, n=3):
    """({kernel name: (launches per call, us per call)}, launches per call) of `n` calls under torch.profiler."""
    import torch
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            call()
        torch.cuda.synchronize()
    agg = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            a = agg.setdefault(e.name, [0, 0.0])
            a[0] += 1
            a[1] += e.device_time
    return {k: (v[0] / n, v[1] / n) for k, v in agg.items()}, sum(v[0] for v in agg.values()) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_chamfer: needs a HIP device (nothing is measured without one)')
    res = {'workload': 'forward + backward of mmd.cd_distance(x1, x2, ChamferDistance(), batch_loss=False), fp32',
           'baseline': 'composed torch ops on the same GPU and tree ([B,N,M,3] differences, sum, min both ways, autograd): the '
                       'parent commit cannot run the op',
           'method': 'one process, alternating windows (composed, op) per round; median ms per call over the windows',
           'rounds': a.rounds, 'window_s': a.window, 'shapes': []}
    for B, N, M in SHAPES:
        calls = _callers(B, N, M)
        ga, gb = calls['op']()
        ca, cb = calls['composed']()
        row = {'B': B, 'N': N, 'M': M,
               'max_abs_grad_difference': max((ga - ca).abs().max().item(), (gb - cb).abs().max().item())}
        k = {}
        for name in ('composed', 'op'):
            for _ in range(WARMUP):
                calls[name]()
            k[name] = max(3, int(a.window / (_window(calls[name], 3) / 1e3) * 1.1) + 1)
        ms = {'composed': [], 'op': []}
        for r in range(a.rounds + 1):                      # the first round is not kept (clocks and the host still settle)
            for name in ('composed', 'op'):
                w = _window(calls[name], k[name])
                if r:
                    ms[name].append(w)
        for name in ('composed', 'op'):
            med = statistics.median(ms[name])
            row[name] = {'ms': round(med, 4), 'spread': round((max(ms[name]) - min(ms[name])) / med, 4),
                         'window_ms': [round(v, 4) for v in ms[name]], 'calls_per_window': k[name]}
        row['speedup'] = round(row['composed']['ms'] / row['op']['ms'], 2)
        calls['sug_chamfer']()
        for name in ('composed', 'op', 'sug_chamfer'):
            kern, launches = _profile(calls[name])
            if name != 'sug_chamfer':
                row[name]['launches_per_call'] = round(launches, 2)
            if name == 'op':
                row['op']['kernels_us'] = {n_: round(v[1], 2) for n_, v in kern.items() if 'chamfer_nn' in n_}
            if name == 'sug_chamfer':
                row['sug_chamfer_kernels_us'] = {n_: [v[0], round(v[1], 2)] for n_, v in kern.items() if 'chamfer' in n_}
        res['shapes'].append(row)
        del calls
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
