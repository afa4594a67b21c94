#!/usr/bin/env python3
"""Forward + backward of mmd.mix_rbf_mmd2_and_ratio (the loss output) on one GPU: the HIP path (ops.mmd_ratio) against the
composed lines of sug_amd/model/mmd.py (_mix_rbf_kernel + _mmd2_and_variance: plain torch ops, the reference's formulation)
on the same device tensors.  Prints one JSON line.

Shapes (m rows per domain, D features): 32 x 266 (a semantic head's feature + label columns), 32 x 4106 and 64 x 4106 (the
node features).  Inputs: X = randn 0.05, Y = randn 0.05 + 0.02, seeded.
Method: one child process times both arms of all shapes -- the arms alternate within a round, `--rounds` rounds, each timing
`--windows` windows of at least `--window` seconds (sized from a short probe after the warm-up) that end in a device
synchronise, profiler off.  Per arm: median ms per call over all windows, and the spread (max - min) / median between the
rounds' medians.  Launches per call (--launches, runs of their own): kernel dispatches of `rocprofv3 --kernel-trace --stats`
runs of 2 and 6 calls after the warm-up, the difference over 4.  The parent process does not touch the GPU.

Usage: python tools/bench_mmd_estimators.py [--rounds 3] [--windows 2] [--window 0.3] [--launches]
                                            [--out profiles/mmd_estimators_bench.json]"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((32, 266), (32, 4106), (64, 4106))
ARMS = ('composed', 'hip')
WARMUP = 5


def _caller(m, D, arm):
    import torch
    from sug_amd.model import mmd
    g = torch.Generator().manual_seed(m * 10000 + D)
    X = (torch.randn(m, D, generator=g) * 0.05).cuda().requires_grad_(True)
    Y = (torch.randn(m, D, generator=g) * 0.05 + 0.02).cuda().requires_grad_(True)

    def hip():
        return mmd.mix_rbf_mmd2_and_ratio(X, Y, mmd.sigma_list, biased=True)[0]

    def composed():
        mmd2, var = mmd._mmd2_and_variance(*mmd._mix_rbf_kernel(X, Y, mmd.sigma_list), biased=True)
        return mmd2 / torch.sqrt(torch.clamp(var, min=mmd.min_var_est))

    fn = hip if arm == 'hip' else composed

    def call():
        X.grad = Y.grad = None
        fn().backward()
    return call


def child_time(rounds, windows, window_s):
    import torch
    calls = {(s, arm): _caller(s[0], s[1], arm) for s in SHAPES for arm in ARMS}
    n = {}
    for key, call in calls.items():
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        n[key] = max(20, int(window_s / ((time.perf_counter() - t) / 20) * 1.1) + 1)
    ms = {key: [] for key in calls}
    for _ in range(rounds):
        for s in SHAPES:
            for arm in ARMS:                                # the arms alternate within a round
                call, k, w = calls[(s, arm)], n[(s, arm)], []
                for _ in range(windows):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(k):
                        call()
                    torch.cuda.synchronize()
                    w.append((time.perf_counter() - t) / k * 1e3)
                ms[(s, arm)].append(w)
    return {'%d,%d,%s' % (s[0], s[1], arm): {'ms': v, 'calls_per_window': n[(s, arm)]} for (s, arm), v in ms.items()}


def child_calls(m, D, arm, count):
    """`count` calls after the warm-up (run under rocprofv3 by the parent process)."""
    import torch
    call = _caller(m, D, arm)
    for _ in range(WARMUP + count):
        call()
    torch.cuda.synchronize()
    return {}


def _child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=limit)
    if r.returncode != 0:
        raise RuntimeError('child %s ended with %d:\n%s' % (args, r.returncode, r.stderr.decode()[-3000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _launches(m, D, arm, count, limit):
    """Kernel dispatches of a run of WARMUP + `count` calls (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='mmd_est_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--child', 'calls', '--shape', '%d,%d' % (m, D), '--arm', arm,
               '--count', str(count)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
        if r.returncode != 0:
            raise RuntimeError('rocprofv3 run ended with %d:\n%s' % (r.returncode, r.stderr.decode()[-3000:]))
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if len(files) != 1:
            raise RuntimeError('expected one kernel_stats.csv, found %s' % files)
        rows = list(csv.DictReader(open(files[0])))
        key = lambda row, *names: next(row[c] for c in row if c.strip().lower() in names)
        return sum(int(key(row, 'calls', 'count')) for row in rows)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--windows', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--child', choices=('time', 'calls'))
    ap.add_argument('--shape')
    ap.add_argument('--arm')
    ap.add_argument('--count', type=int, default=2)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, HERE)
        if a.child == 'time':
            print(json.dumps(child_time(a.rounds, a.windows, a.window)))
        else:
            m, D = (int(v) for v in a.shape.split(','))
            print(json.dumps(child_calls(m, D, a.arm, a.count)))
        return
    res = {'workload': 'forward + backward of mix_rbf_mmd2_and_ratio (loss), biased, sigma list of 5, X = randn 0.05, '
                       'Y = randn 0.05 + 0.02', 'dtype': 'fp32',
           'arms': {'composed': 'the composed torch lines of sug_amd/model/mmd.py on device tensors (eager)',
                    'hip': 'ops.mmd_ratio (sug_mmd_ratio_fwd / _bwd), eager launches'},
           'rounds': a.rounds, 'windows_per_round': a.windows, 'window_s': a.window, 'results': []}
    failed = None
    try:
        timed = _child(['--child', 'time', '--rounds', str(a.rounds), '--windows', str(a.windows), '--window', str(a.window)], 600)
        for m, D in SHAPES:
            row = {'m': m, 'D': D}
            for arm in ARMS:
                r = timed['%d,%d,%s' % (m, D, arm)]
                flat = [v for w in r['ms'] for v in w]
                med = statistics.median(flat)
                per_round = [statistics.median(w) for w in r['ms']]
                row['ms_' + arm] = round(med, 4)
                row['spread_between_rounds_' + arm] = round((max(per_round) - min(per_round)) / med, 4)
                row['round_medians_ms_' + arm] = [round(v, 4) for v in per_round]
                row['calls_per_window_' + arm] = r['calls_per_window']
            res['results'].append(row)
        if a.launches:
            for row in res['results']:                      # (a child that fails may have faulted the GPU: the except ends it all)
                for arm in ARMS:
                    lo, hi = (_launches(row['m'], row['D'], arm, c, 300) for c in (2, 6))
                    row['launches_per_call_' + arm] = round((hi - lo) / 4, 2)
    except (RuntimeError, StopIteration, subprocess.TimeoutExpired) as e:
        failed = res['error'] = str(e)[-800:]
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)
    if failed is not None:
        sys.exit(1)


if __name__ == '__main__':
    main()
