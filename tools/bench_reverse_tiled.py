#!/usr/bin/env python3
"""Kernel time of the tiled reverse-list build (sug_reverse_lists_tiled), device events, the variants of a row alternated in
one process, the median of ROUNDS rounds with the spread (max - min of the rounds).  Every variant is captured REPS times
into one graph and the replay is timed (tools/bench_reverse.py's method: the figure is device time, not the launch rate of
the Python caller); a variant that cannot be captured is timed as REPS eager calls between two events and says so.

  (a) beyond the LDS build: B = 16, N = 2048, k = 20 and k = 32, kNN graphs of random clouds.  tiled | torch, the composed
      torch form of the same int32 arrays on the same GPU, the only other way to these lists at these sizes: stable argsort,
      counts by scatter_add (torch.bincount waits for the host to size its output), cumsum, the two casts to int32.
      `faster_beyond_spreads`: torch - tiled > the two spreads added.
  (b) what the dispatcher's choice is worth, for information: the tiled build forced (library's tile) at two shapes both
      builds take, 64 x 1024 x 20 and the LDS build's largest at N = 2048, against the LDS build.

    python tools/bench_reverse_tiled.py [--out profiles/reverse_tiled_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sug_amd import ops

REPS, ROUNDS = 20, 7


def torch_form(idx, N):
    B, E = idx.shape
    key = idx.long()
    ent = torch.argsort(key, dim=1, stable=True).to(torch.int32)
    counts = torch.zeros(B, N, dtype=torch.long, device=idx.device).scatter_add_(1, key, torch.ones_like(key))
    off = torch.cat((torch.zeros(B, 1, dtype=torch.long, device=idx.device), counts.cumsum(1)), 1).to(torch.int32)
    return off, ent


def timer(fn):
    """-> (a callable returning microseconds per call, 'graph' | 'eager')."""
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph, how = torch.cuda.CUDAGraph(), 'graph'
    try:
        with ops.capture_guard(), torch.cuda.graph(graph):
            for _ in range(REPS):
                fn()
        run = graph.replay
    except Exception:       # noqa: BLE001 -- a torch op that does not capture is timed eagerly
        torch.cuda.synchronize()
        how = 'eager'

        def run():
            for _ in range(REPS):
                fn()
    run()
    torch.cuda.synchronize()

    def once():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / REPS
    return once, how


def alternate(variants):
    timers = {k: timer(f) for k, f in variants.items()}
    us = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, (once, _) in timers.items():
            us[k].append(once())
    out = {}
    for k, v in us.items():
        out[k + '_us'] = round(sorted(v)[ROUNDS // 2], 2)
        out[k + '_us_spread'] = round(max(v) - min(v), 2)
        out[k + '_us_rounds'] = [round(x, 2) for x in v]
        out[k + '_timed'] = timers[k][1]
    return out


def knn_lists(B, N, k, seed):
    g = torch.Generator().manual_seed(seed)
    return ops.knn(torch.rand(B, N, 3, generator=g).cuda(), k).reshape(B, N * k).contiguous()


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'workload': 'tiled reverse-list build: (a) against the composed torch form beyond the LDS build, (b) forced, against '
                       'the LDS build', 'reps_per_replay': REPS, 'rounds': ROUNDS, 'beyond_lds': [], 'both_builds': []}
    for B, N, k in ((16, 2048, 20), (16, 2048, 32)):
        idx = knn_lists(B, N, k, 1)
        assert same(ops.reverse_lists_tiled(idx, N), torch_form(idx, N))
        row = alternate({'tiled': lambda: ops.reverse_lists_tiled(idx, N), 'torch': lambda: torch_form(idx, N)})
        row.update(B=B, N=N, k=k, entries_per_cloud=N * k, speedup=round(row['torch_us'] / row['tiled_us'], 2),
                   faster_beyond_spreads=bool(row['torch_us'] - row['tiled_us'] > row['torch_us_spread'] + row['tiled_us_spread']))
        res['beyond_lds'].append(row)
    g = torch.Generator().manual_seed(2)
    for name, (B, E, N) in (('bench', (64, 1024 * 20, 1024)), ('max_n2048', (2, 40416, 2048))):
        idx = knn_lists(B, N, 20, 3) if name == 'bench' else torch.randint(0, N, (B, E), generator=g, dtype=torch.int32).cuda()
        assert same(ops.reverse_lists_tiled(idx, N), ops.reverse_lists(idx, N))
        row = alternate({'tiled': lambda: ops.reverse_lists_tiled(idx, N), 'lds': lambda: ops.reverse_lists(idx, N)})
        row.update(shape=name, B=B, E=E, N=N, tiled_over_lds=round(row['tiled_us'] / row['lds_us'], 2))
        res['both_builds'].append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
