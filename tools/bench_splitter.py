#!/usr/bin/env python3
"""Geometric sub-domain splitter: what one anchor try costs on the device, and what the same registrations cost on the host.

    python tools/bench_splitter.py [--launches 20] [--out profiles/splitter_bench.json]
    python tools/bench_splitter.py --host-baseline      # (b) alone; the full run starts it as a child process
    python tools/bench_splitter.py --launch-only        # (c)'s workload; the full run starts it under rocprofv3

(a) One anchor try of split_dataset_geometric: ops.icp_fitness of one anchor against M = 1024 synthetic clouds of 500 points
    (the three families of tests/splitter_cases.py, through normal_pc), one launch.  Device events around each of
    `launches` launches after a warm-up; the median.  From the per-pair iteration counts the launch's fp64 operations:
    every pair runs iters + 1 evaluations of Ns x Nt distance tests at 8 flops each (3 subtractions, 3 products, 2 sums;
    the compare and the reductions are not counted), over the median time = achieved FLOP/s.
(b) The numpy fp64 restatement (tests/splitter_cases.icp) of the same 1024 registrations on 16 host processes, one numpy
    thread each, in a child process that never opens the GPU.  open3d, whose registration_icp the reference calls once per
    cloud, is not installed here and could NOT be timed; the restatement evaluates a dense 500 x 500 distance matrix where
    open3d searches a KD-tree, so this is the cost of the restatement, not of the reference tool.
(c) The kernel's time from a rocprofv3 --kernel-trace --stats run of its own (a child that only launches the kernel).
No time here is an acceptance condition: there was no such path before."""
import argparse
import csv
import glob
import json
import multiprocessing
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

M, N_POINTS, ANCHOR = 1024, 500, 300
HOST_PROCESSES = 16


def synth_clouds():
    import splitter_cases as C
    g = np.random.default_rng(2024)
    return np.stack([C.make_cloud(C.FAMILIES[i % 3], N_POINTS, g) for i in range(M)])


def _host_pair(args):
    import splitter_cases as C
    count, _, iters, _ = C.icp(*args)
    return count, iters


def host_baseline(a):
    clouds = synth_clouds()
    with multiprocessing.Pool(HOST_PROCESSES) as pool:
        pool.map(_host_pair, [(clouds[ANCHOR], clouds[i]) for i in range(HOST_PROCESSES)])          # start the workers
        t0 = time.perf_counter()
        res = pool.map(_host_pair, [(clouds[ANCHOR], c) for c in clouds], chunksize=8)
        dt = time.perf_counter() - t0
    print(json.dumps({'host_restatement': {'seconds': dt, 'pairs': M, 'processes': HOST_PROCESSES, 'pairs_per_s': M / dt,
                                           'count': [int(r[0]) for r in res], 'iters': [int(r[1]) for r in res],
                                           'open3d': 'not installed: could not be timed'}}))


def device_inputs(dev):
    clouds = torch.from_numpy(synth_clouds()).to(dev)
    return clouds[ANCHOR].contiguous(), clouds


def launch_only(a):
    from sug_amd import ops
    src, tgt = device_inputs(torch.device('cuda:0'))
    for _ in range(a.launches):
        ops.icp_fitness(src, tgt)
    torch.cuda.synchronize()


def kernel_trace(a):
    """rocprofv3 around a child that only launches the kernel -> its row of the kernel statistics."""
    d = tempfile.mkdtemp(prefix='splitter_trace_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'p', '--', sys.executable,
               os.path.abspath(__file__), '--launch-only', '--launches', str(a.launches)]
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return {'error': 'rocprofv3 exit %d: %s' % (r.returncode, r.stderr[-300:].strip())}
        rows = [row for row in csv.DictReader(open(files[0])) if 'icp_fitness_kernel' in row.get('Name', '')]
        if not rows:
            return {'error': 'no icp_fitness_kernel row in %s' % os.path.basename(files[0])}
        row = rows[0]
        return {'name': row['Name'], 'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3,
                'min_us': float(row['MinNs']) / 1e3, 'max_us': float(row['MaxNs']) / 1e3}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def device_try(a, dev):
    from sug_amd import ops
    src, tgt = device_inputs(dev)
    for _ in range(3):
        count, rmse, iters, _ = ops.icp_fitness(src, tgt)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.icp_fitness(src, tgt)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = sorted(times)[len(times) // 2]
    iters, count = iters.cpu().numpy(), count.cpu().numpy()
    flops = float((iters.astype(np.int64) + 1).sum()) * N_POINTS * N_POINTS * 8
    return {'M': M, 'points': N_POINTS, 'launches': a.launches, 'ms_median': med, 'ms_min': min(times), 'ms_max': max(times),
            'pairs_per_s': M / (med * 1e-3), 'evaluations': int((iters.astype(np.int64) + 1).sum()),
            'fp64_flops_per_launch': flops, 'achieved_fp64_TFLOPs': flops / (med * 1e-3) / 1e12,
            'iteration_histogram': np.bincount(iters, minlength=31).tolist(), 'mean_fitness': float(count.mean() / N_POINTS),
            'count': count.tolist(), 'iters': iters.tolist()}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--host-baseline', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--skip-trace', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'splitter_bench.json'))
    a = ap.parse_args()
    if a.host_baseline:
        host_baseline(a)
        sys.exit(0)
    if a.launch_only:
        launch_only(a)
        sys.exit(0)
    result = {}
    if not a.skip_host:              # first, in a child: this process has not touched the GPU yet
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--host-baseline'], capture_output=True, text=True,
                               timeout=900, env=dict(os.environ, HIP_VISIBLE_DEVICES='', OMP_NUM_THREADS='1'))
        if child.returncode != 0:
            raise RuntimeError('host baseline failed:\n' + child.stderr[-2000:])
        result.update(json.loads(child.stdout.strip().splitlines()[-1]))
    if not a.skip_trace:             # also before this process opens the GPU
        result['kernel_trace'] = kernel_trace(a)
        if 'error' in result['kernel_trace']:      # the kernel time is one of the recorded figures: no file without it
            sys.exit('bench_splitter: kernel trace failed (%s); --skip-trace runs without it' % result['kernel_trace']['error'])
    if not torch.cuda.is_available():
        raise RuntimeError('bench_splitter needs a HIP device; there is no CPU path for (a)')
    dev = torch.device('cuda:0')
    result['device'] = torch.cuda.get_device_name(0)
    result['anchor_try'] = device_try(a, dev)
    host = result.get('host_restatement')
    if host:                          # how far the two agree: the full-run tolerance of the tests, at this size
        same = sum(c == d and i == j for c, d, i, j in zip(host.pop('count'), result['anchor_try']['count'],
                                                           host.pop('iters'), result['anchor_try']['iters']))
        result['pairs_with_equal_count_and_iters'] = same
        host['speedup_of_the_launch'] = host['seconds'] / (result['anchor_try']['ms_median'] * 1e-3)
    del result['anchor_try']['count'], result['anchor_try']['iters']
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
