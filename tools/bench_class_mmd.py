#!/usr/bin/env python3
"""The class-aligned MMD modes (HARD_MMD; MAX_HARD_MMD with PAIRING: stable) in a SUGStep on one GPU: what choosing the rows on
the device (ops.class_mmd) buys over the composed path (boolean indexing / host-built index lists).  Prints one JSON line.

Workload: DGCNN, 32 clouds per domain, N = 1024, bench.BENCH_METHODS with the NAME of both MMD entries replaced; fresh random
labels every step, drawn on the device (so n changes from step to step and the label draw itself waits for nothing); row 0
of the two domains shares its label, so that n >= 1 (the composed hard_mmd raises on a batch without a pair).
Configurations: `hard` (HARD_MMD) and `max_hard` (MAX_HARD_MMD + PAIRING: stable; the composed arm runs MAX_HARD_MMD with the
default host pairing, which is what the key meant before 'stable' existed).
Arms, each in a child process of its own (SUG_CLASS_MMD is read at import):
  composed  SUG_CLASS_MMD=0, eager launches: a step configured this way cannot be captured (nonzero / .cpu() wait for the device;
            UDAStep records a refusal and stays eager, SUGStep's capture raises), so eager is how it runs
  eager     ops.class_mmd, use_graph=False
  replay    ops.class_mmd, use_graph=True (planned, captured and replayed before any clock starts)
Method: the arms alternate within a round, `--rounds` rounds; a child warms up, sizes a window to at least `--window` seconds
from a short probe and times `--windows` windows that end in a device synchronise, profiler off.  Per arm: median ms per step
over all windows of all rounds, and the spread (max - min) / median between the rounds' medians.  Host waits per step: warnings of
torch.cuda.set_sync_debug_mode('warn') over 4 further steps (synchronising torch calls; the ctypes launches never wait).
Launches per step (--launches, runs of their own): kernel dispatches of `rocprofv3 --kernel-trace --stats` runs of 2 and 6
steps after the warm-up, the difference over 4.  The parent process does not touch the GPU.

Usage: python tools/bench_class_mmd.py [--configs hard,max_hard] [--rounds 3] [--windows 2] [--window 0.5] [--launches]
                                       [--out profiles/class_mmd_bench.json]"""
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
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B, MODEL = 1024, 32, 'DGCNN'
WARMUP = 4
ARMS = ('composed', 'eager', 'replay')


def _stepper(config, arm):
    import torch
    import bench
    from oracle import ref_cpu as O
    from sug_amd import ops
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    assert ops.CLASS_MMD == (arm != 'composed')
    name = {'NAME': 'HARD_MMD'} if config == 'hard' else {'NAME': 'MAX_HARD_MMD'}
    if config == 'max_hard' and arm != 'composed':
        name['PAIRING'] = 'stable'
    methods = {k: [dict(bench.BENCH_METHODS[k][0], **name)] for k in ('GEO_MMD', 'SEM_MMD')}
    torch.manual_seed(0)
    net = Net_MDA(MODEL).cuda().train()
    g = torch.Generator().manual_seed(0)
    data, data_t = O.synth_clouds(B, N, g).cuda(), O.synth_clouds(B, N, g).cuda()
    tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=(arm == 'replay'), methods=methods)
    dg = torch.Generator(device='cuda').manual_seed(1)

    def step():
        lab = torch.randint(0, 10, (B,), generator=dg, device='cuda')
        lab_t = torch.randint(0, 10, (B,), generator=dg, device='cuda')
        lab_t[0] = lab[0]                                   # n >= 1: without a pair the composed hard_mmd raises
        return tr.step(data, lab, data_t, lab_t)

    def end():
        if arm == 'replay' and (len(tr._graphs) != 1 or next(iter(tr._graphs.values()))['graph'] is None):
            raise RuntimeError('%s/replay did not replay one graph' % config)
    return step, end


def child_time(config, arm, windows, window_s):
    import torch
    step, end = _stepper(config, arm)
    for _ in range(WARMUP):
        step()
    end()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    probe = (time.perf_counter() - t) / 10
    n = max(10, int(window_s / probe * 1.1) + 1)
    ms = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) / n * 1e3)
    end()
    waits = None
    try:
        torch.cuda.set_sync_debug_mode('warn')
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            for _ in range(4):
                step()
        waits = sum('synchroniz' in str(w.message).lower() for w in seen) / 4.0
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return {'ms': ms, 'steps_per_window': n, 'host_waits_per_step': waits}


def child_steps(config, arm, steps):
    """`steps` steps after the warm-up (run under rocprofv3 by the parent process)."""
    import torch
    step, end = _stepper(config, arm)
    for _ in range(WARMUP + steps):
        step()
    end()
    torch.cuda.synchronize()
    return {}


def _env(arm):
    env = dict(os.environ)
    env['SUG_CLASS_MMD'] = '0' if arm == 'composed' else '1'
    return env


def _child(args, limit, env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=limit, env=env)
    if r.returncode != 0:
        raise RuntimeError('child %s ended with %d:\n%s' % (args, r.returncode, r.stderr.decode()[-3000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _launches(config, arm, steps, limit):
    """Kernel dispatches of a run of WARMUP + `steps` steps (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='class_mmd_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--child', 'steps', '--config', config, '--arm', arm, '--steps', str(steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, env=_env(arm))
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
    ap.add_argument('--configs', default='hard,max_hard')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--windows', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--child', choices=('time', 'steps'))
    ap.add_argument('--config')
    ap.add_argument('--arm')
    ap.add_argument('--steps', type=int, default=2)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, HERE)
        fn = {'time': lambda: child_time(a.config, a.arm, a.windows, a.window),
              'steps': lambda: child_steps(a.config, a.arm, a.steps)}[a.child]
        print(json.dumps(fn()))
        return
    res = {'workload': 'SUGStep with class-aligned MMD terms, %s %d per domain, N = %d, random labels per step' % (MODEL, B, N),
           'dtype': 'fp32', 'arms': {'composed': 'SUG_CLASS_MMD=0, eager launches (the composed path cannot be captured)',
                                     'eager': 'ops.class_mmd, use_graph=False', 'replay': 'ops.class_mmd, use_graph=True'},
           'rounds': a.rounds, 'windows_per_round': a.windows, 'window_s': a.window, 'results': []}
    failed = None
    for config in a.configs.split(','):
        if failed is not None:                              # a child that failed may have faulted the GPU: start nothing more
            break
        row = {'config': config}
        try:
            ms = {arm: [] for arm in ARMS}
            waits = {}
            for _ in range(a.rounds):
                for arm in ARMS:                            # the arms alternate within a round
                    r = _child(['--child', 'time', '--config', config, '--arm', arm, '--windows', str(a.windows),
                                '--window', str(a.window)], 300, _env(arm))
                    ms[arm].append(r['ms'])
                    waits[arm] = r['host_waits_per_step']
            for arm in ARMS:
                flat = [v for w in ms[arm] for v in w]
                med = statistics.median(flat)
                per_round = [statistics.median(w) for w in ms[arm]]
                row['ms_' + arm] = round(med, 4)
                row['spread_between_rounds_' + arm] = round((max(per_round) - min(per_round)) / med, 4)
                row['round_medians_ms_' + arm] = [round(v, 4) for v in per_round]
                row['host_waits_per_step_' + arm] = waits[arm]
            if a.launches:
                for arm in ARMS:
                    lo, hi = (_launches(config, arm, s, 300) for s in (2, 6))
                    row['launches_per_step_' + arm] = round((hi - lo) / 4, 2)
        except (RuntimeError, StopIteration, subprocess.TimeoutExpired) as e:
            failed = row['error'] = str(e)[-800:]
        res['results'].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)
    if failed is not None:
        sys.exit(1)


if __name__ == '__main__':
    main()
