#!/usr/bin/env python3
"""Point Feature Histograms: what the descriptors of a dataset and one anchor-against-all distance cost on the device, and
what the numpy restatement of the same work costs on the host.

    python tools/bench_pfh.py [--launches 10] [--out profiles/pfh_bench.json]
    python tools/bench_pfh.py --host-baseline       # (c) alone; the full run starts it as a child process

(a) sug_pfh_descriptors on M = 4096 clouds of 500 points with the reference's parameters (rad 0.2, 8 neighbours, div 2):
    shells drawn on the device and taken through process_pts, as utils/pfh.py's __main__ does with its datasets.  One launch.
(b) sug_pfh_hist_distance of one anchor's histograms against all 4096 (the splitter's distance_of).  One launch.
    (a) and (b) are timed ALTERNATELY with device events around each launch after a warm-up of both; the medians.
    Algorithmic work, from the shapes and the neighbour counts (kept here, next to the timing):
      (a) (k + 1) sweeps of N x N distance tests at 9 fp64 operations (3 differences, 3 products, 2 sums, 1 square root)
          -- the selection this kernel chose; a single sweep with a kept list would need N x N -- plus 93 per pair feature
          set; bytes: the cloud in, the five outputs out.
      (b) Ns x Nt x 3D + Ns x Nt (a difference, a product, a sum per bin; a square root per pair of rows); bytes: all
          histograms and counts in once, one fp64 out per pair.
    The time is held against the larger of operations / 78.6 TFLOP/s (the MI355X's fp64 vector rate) and bytes / 8 TB/s.
(c) The numpy fp64 restatement (tests/pfh_cases.py) of the same two computations on HOST_CLOUDS clouds over 16 host
    processes, one numpy thread each, in a child process that never opens the GPU; scaled per cloud to 4096.  The
    restatement is vectorised numpy, far faster than the reference's Python loops over np.matrix (seconds per cloud): this
    is the cost of the restatement, not of the reference tool.
No time here is an acceptance condition: there was no such path before."""
import argparse
import json
import multiprocessing
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

M, RAW_POINTS, N_POINTS, ANCHOR = 4096, 2000, 500, 1300
RAD, K, DIV = 0.2, 8, 2
HOST_CLOUDS, HOST_PROCESSES = 64, 16
PEAK_FP64, PEAK_BYTES = 78.6e12, 8.0e12


def _host_distance(args):
    import pfh_cases as C
    (hs, cs), (ht, ct) = args
    return C.hist_distance(hs, cs > 0, ht, ct > 0)


def _host_cloud(seed):
    import pfh_cases as C
    return C.shell(N_POINTS, np.random.default_rng(seed))


def _host_describe(cloud):
    import pfh_cases as C
    r = C.descriptors(cloud, RAD, K, DIV)
    return r['hist'], r['cnt']


def host_baseline(a):
    with multiprocessing.Pool(HOST_PROCESSES) as pool:
        clouds = pool.map(_host_cloud, range(HOST_CLOUDS))                                   # also starts the workers
        t0 = time.perf_counter()
        desc = pool.map(_host_describe, clouds)
        t_desc = time.perf_counter() - t0
        t0 = time.perf_counter()
        pool.map(_host_distance, [(desc[0], d) for d in desc])
        t_dist = time.perf_counter() - t0
    print(json.dumps({'host_restatement': {
        'clouds': HOST_CLOUDS, 'processes': HOST_PROCESSES, 'descriptors_seconds': t_desc, 'distances_seconds': t_dist,
        'scaling': 'seconds * %d / %d: the work per cloud does not depend on the other clouds' % (M, HOST_CLOUDS),
        'descriptors_seconds_scaled_to_4096': t_desc * M / HOST_CLOUDS,
        'distances_seconds_scaled_to_4096': t_dist * M / HOST_CLOUDS}}))


def device_clouds(dev):
    from sug_amd.dataset_splitter import process_pts
    g = torch.Generator(device=dev).manual_seed(2026)
    out = []
    for _ in range(M // 512):                                     # in slices: the raw clouds are four times the result
        v = torch.randn(512, RAW_POINTS, 3, device=dev, generator=g)
        v = v / v.norm(dim=2, keepdim=True)
        scale = 0.7 + 0.3 * torch.rand(512, RAW_POINTS, 1, device=dev, generator=g)
        out.append(process_pts(v * scale * torch.tensor([1.0, 0.7, 0.5], device=dev), N_POINTS))
    return torch.cat(out)


def measure(a, dev):
    from sug_amd import ops
    clouds = device_clouds(dev)
    for _ in range(2):
        hist, _, _, cnt, used = ops.pfh_descriptors(clouds, RAD, K, DIV)
        ops.pfh_hist_distance(hist[ANCHOR], cnt[ANCHOR], hist, cnt)
    torch.cuda.synchronize()
    t_desc, t_dist = [], []
    for _ in range(a.launches):                                   # alternated: both see the same neighbours on the machine
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        hist, _, _, cnt, used = ops.pfh_descriptors(clouds, RAD, K, DIV)
        e[1].record()
        e[2].record()
        d = ops.pfh_hist_distance(hist[ANCHOR], cnt[ANCHOR], hist, cnt)
        e[3].record()
        torch.cuda.synchronize()
        t_desc.append(e[0].elapsed_time(e[1]))
        t_dist.append(e[2].elapsed_time(e[3]))
    med = lambda t: sorted(t)[len(t) // 2]
    c = cnt.cpu().numpy().astype(np.int64)
    pairs = int(((c + 1) * c // 2).sum())
    D = DIV ** 3
    ops_desc = float(M) * (K + 1) * N_POINTS * N_POINTS * 9 + pairs * 93.0
    bytes_desc = float(M) * N_POINTS * (12 + D * 8 + 24 + 4 * K + 4) + 4 * M
    rows_used = (c > 0).sum(axis=1)
    ops_dist = float((rows_used[ANCHOR] * rows_used).sum()) * (3 * D + 1)
    bytes_dist = float(M) * N_POINTS * (D * 8 + 4) + N_POINTS * (D * 8 + 4) + 8 * M

    def entry(times, flops, nbytes):
        t = med(times) * 1e-3
        floor_ops, floor_bytes = flops / PEAK_FP64, nbytes / PEAK_BYTES
        return {'ms_median': med(times), 'ms_min': min(times), 'ms_max': max(times), 'launches': len(times),
                'fp64_operations': flops, 'bytes': nbytes, 'achieved_fp64_TFLOPs': flops / t / 1e12, 'achieved_GBps': nbytes / t / 1e9,
                'bound': 'operations' if floor_ops >= floor_bytes else 'bytes', 'floor_ms': max(floor_ops, floor_bytes) * 1e3,
                'share_of_floor': max(floor_ops, floor_bytes) / t}
    dist = d.cpu().numpy()
    return {'M': M, 'points': N_POINTS, 'rad': RAD, 'nneighbors': K, 'div': DIV,
            'clouds_with_every_point_used': int((used.cpu().numpy() == N_POINTS).sum()), 'mean_neighbours': float(c.mean()),
            'pairs': pairs, 'descriptors': entry(t_desc, ops_desc, bytes_desc), 'hist_distance': entry(t_dist, ops_dist, bytes_dist),
            'distance_min_median_max': [float(np.nanmin(dist)), float(np.nanmedian(dist)), float(np.nanmax(dist))],
            'clouds_per_s': M / (med(t_desc) * 1e-3)}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--host-baseline', action='store_true')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pfh_bench.json'))
    a = ap.parse_args()
    if a.host_baseline:
        host_baseline(a)
        sys.exit(0)
    result = {}
    if not a.skip_host:               # first, in a child: this process has not touched the GPU yet
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--host-baseline'], capture_output=True, text=True,
                               timeout=900, env=dict(os.environ, HIP_VISIBLE_DEVICES='', OMP_NUM_THREADS='1'))
        if child.returncode != 0:
            raise RuntimeError('host baseline failed:\n' + child.stderr[-2000:])
        result.update(json.loads(child.stdout.strip().splitlines()[-1]))
    if not torch.cuda.is_available():
        raise RuntimeError('bench_pfh needs a HIP device; there is no CPU path for (a) and (b)')
    dev = torch.device('cuda:0')
    result['device'] = torch.cuda.get_device_name(0)
    result['launches'] = measure(a, dev)
    host = result.get('host_restatement')
    if host:
        host['descriptors_speedup_of_the_launch'] = host['descriptors_seconds_scaled_to_4096'] / (result['launches']['descriptors']['ms_median'] * 1e-3)
        host['distances_speedup_of_the_launch'] = host['distances_seconds_scaled_to_4096'] / (result['launches']['hist_distance']['ms_median'] * 1e-3)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
