#!/usr/bin/env python3
"""The source-only training step (train_source.py:113-131) of the four capturable classifiers on one GPU.  Prints one JSON line.

Arms, per classifier and batch size:
  a  the caller's eager loop: model(data), nn.CrossEntropyLoss, backward, sug_amd.optim.Adam step, zero_grad, loss.item() and the
     two running totals every step (nothing but the API the package had before SourceStep: runs unchanged on an older tree);
  b  SourceStep(use_graph=False): the same step with ops.ce and the device-resident totals, launched eagerly;
  c  SourceStep(use_graph=True): planned, captured, replayed.
Sizes: Pointnet_cls B = 8 (BASELINE configuration 1) and B = 64, DGCNN and Pointnet2_cls B = 64, PointTransformerCls B = 32;
N = 1024.

Method: a fresh child process per (classifier, arm, round); the arms alternate within a round, the rounds repeat.  A child
warms its one key up (the graph arm: planned, captured and replayed before any clock starts), sizes a window to at least
`--window` seconds from a short probe, and times `--windows` device-synchronised windows with the profiler off (arms b / c read
epoch_totals() once per window, inside it).  Reported per arm: the median ms per step over all windows of all rounds and the
window-to-window spread (max - min) / median.  Launches per step: `rocprofv3 --kernel-trace --stats` runs of 2 and 6 steps
after the warm-up, the difference over 4 (--launches; a run of its own).
The parent process does not touch the GPU.

Usage: python tools/bench_source_step.py [--arms a,b,c] [--configs Pointnet_cls:8,...] [--rounds 2] [--windows 3]
                                         [--window 1.0] [--launches] [--out FILE]"""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1024
CONFIGS = [('Pointnet_cls', 8), ('Pointnet_cls', 64), ('DGCNN', 64), ('Pointnet2_cls', 64), ('PointTransformerCls', 32)]
WARMUP = 4


def _setup(name, B):
    import torch
    from oracle import ref_cpu as O
    from sug_amd.model import model_pointnet as MP
    torch.manual_seed(0)
    if name == 'PointTransformerCls':
        from sug_amd.model.Ptran_model import PointTransformerCls
        net = PointTransformerCls()
    else:
        net = getattr(MP, name)()
    net = net.cuda().train()
    g = torch.Generator().manual_seed(0)
    x = O.synth_clouds(B, N, g).cuda()
    lab = torch.randint(0, 10, (B,), generator=g).cuda()
    return net, x, lab


def _stepper(name, B, arm):
    """(step(), window_end()) of an arm."""
    import torch
    net, x, lab = _setup(name, B)
    if arm == 'a':
        from sug_amd.optim import Adam
        crit = torch.nn.CrossEntropyLoss().cuda()
        opt = Adam(net.parameters(), lr=1e-3, weight_decay=5e-5)
        tot = [0.0, 0]

        def step():
            loss = crit(net(x), lab)
            loss.backward()
            opt.step()
            opt.zero_grad()
            tot[0] += loss.item() * x.size(0)
            tot[1] += x.size(0)
        return step, lambda: None
    from sug_amd.source_step import SourceStep
    tr = SourceStep(net, lr=1e-3, weight_decay=5e-5, use_graph=(arm == 'c'))

    def end():
        tr.epoch_totals()
        if arm == 'c' and (tr.stats['captured'] != 1 or tr.stats['refused']):
            raise RuntimeError('arm c did not replay: %s (%s)' % (tr.stats, tr.why))
    return (lambda: tr.step(x, lab)), end


def child_time(name, B, arm, windows, window_s):
    import torch
    step, end = _stepper(name, B, arm)
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
        end()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) / n * 1e3)
    return {'ms': ms, 'steps_per_window': n}


def child_steps(name, B, arm, steps):
    """`steps` steps after the warm-up (run under rocprofv3 by the parent)."""
    import torch
    step, end = _stepper(name, B, arm)
    for _ in range(WARMUP + steps):
        step()
    end()
    torch.cuda.synchronize()
    return {}


def _child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=limit)
    if r.returncode != 0:
        raise RuntimeError('child %s ended with %d:\n%s' % (args, r.returncode, r.stderr.decode()[-3000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _launches(name, B, arm, steps, limit):
    """Kernel dispatches of a run of WARMUP + `steps` steps (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='source_step_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--child', 'steps', '--model', name, '--B', str(B), '--arm', arm,
               '--steps', str(steps)]
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
    ap.add_argument('--arms', default='a,b,c')
    ap.add_argument('--configs', default=','.join('%s:%d' % c for c in CONFIGS))
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--no-time', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--child', choices=('time', 'steps'))
    ap.add_argument('--model')
    ap.add_argument('--B', type=int)
    ap.add_argument('--arm')
    ap.add_argument('--steps', type=int, default=2)
    a = ap.parse_args()
    if a.child:
        fn = {'time': lambda: child_time(a.model, a.B, a.arm, a.windows, a.window),
              'steps': lambda: child_steps(a.model, a.B, a.arm, a.steps)}[a.child]
        print(json.dumps(fn()))
        return
    arms = a.arms.split(',')
    configs = [(c.split(':')[0], int(c.split(':')[1])) for c in a.configs.split(',')]
    res = {'workload': 'source-only train step (train_source.py:113-131)', 'N': N, 'dtype': 'fp32', 'arms': {
        'a': 'caller\'s eager loop, sug_amd.optim.Adam, loss.item() every step', 'b': 'SourceStep(use_graph=False)',
        'c': 'SourceStep(use_graph=True)'}, 'rounds': a.rounds, 'windows_per_round': a.windows, 'window_s': a.window,
        'results': []}
    failed = None
    for name, B in configs:
        if failed is not None:                              # a child that failed may have faulted the GPU: start nothing more
            break
        row = {'model': name, 'B': B}
        if not a.no_time:
            ms = {arm: [] for arm in arms}
            for _ in range(a.rounds):
                for arm in arms:                            # the arms alternate within a round
                    r = _child(['--child', 'time', '--model', name, '--B', str(B), '--arm', arm, '--windows', str(a.windows),
                                '--window', str(a.window)], 600)
                    ms[arm] += r['ms']
            for arm in arms:
                med = statistics.median(ms[arm])
                row['ms_' + arm] = round(med, 4)
                row['spread_' + arm] = round((max(ms[arm]) - min(ms[arm])) / med, 4)
                row['windows_ms_' + arm] = [round(v, 4) for v in ms[arm]]
            if 'a' in arms and 'c' in arms:
                row['speedup_c_over_a'] = round(row['ms_a'] / row['ms_c'], 3)
        if a.launches:
            for arm in arms:
                try:
                    lo, hi = _launches(name, B, arm, 2, 600), _launches(name, B, arm, 6, 600)
                except (RuntimeError, StopIteration, subprocess.TimeoutExpired) as e:
                    failed = row['launches_error_' + arm] = str(e)[-500:]
                    break
                row['launches_per_step_' + arm] = round((hi - lo) / 4, 2)
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
