#!/usr/bin/env python3
"""Class counts other than ten on one GPU: what the run-time class count costs at ten classes (nothing is expected: the same
kernels launch), what the 64-wide instantiation of the fused heads' backward buys a 40-class model over the composed head,
and the SDA weights of three 40-class heads in one launch against the composed torch lines.  Prints one JSON line.

Workload of (a) and (b): SUGStep, DGCNN, 32 clouds per domain, N = 1024, bench.BENCH_METHODS, graph replay (planned, captured
and replayed before any clock starts), fixed clouds and labels drawn over the full range.
  (a) c10          Net_MDA('DGCNN'), ten classes, on this tree -- and with --parent DIR (a built checkout of the parent commit)
      c10_parent   the same step on that tree, alternated with c10
  (b) c40_fused    Net_MDA('DGCNN', num_class=40): the heads' last layer through sug_head_linear_* (backward: the 64-wide
                   instantiation)
      c40_composed the same model with SUG_HEADS_FUSED=0: library GEMMs + LayerNorm / dropout ops (the parent cannot build
                   a 40-class model; before this instantiation a 40-class model ran this head in every step)
  (c) sda_multi    ops.sda_prob_weights_multi of three heads, C = 40, m = 32, 'mean2one': one launch
      sda_composed the lines of mmd.prob_weights_soft's fallback (softmax, cat, normalise, two KL terms, distance2weights) from
                   torch ops on the device, three times
Method: the arms of a group alternate within a round, `--rounds` rounds, each arm in a child process of its own (SUG_HEADS_FUSED
is read at import); a child warms up, sizes a window to at least `--window` seconds from a short probe and times `--windows`
windows that end in a device synchronise, profiler off.  Per arm: median ms per step (us per call for (c)) over all windows of
all rounds, and the spread (max - min) / median between the rounds' medians.  Launches per step (--launches, runs of their
own): kernel dispatches of `rocprofv3 --kernel-trace --stats` runs of 2 and 6 steps after the warm-up, the difference over 4.
The parent process does not touch the GPU.

Usage: python tools/bench_num_class.py [--parent DIR] [--rounds 3] [--windows 2] [--window 0.5] [--launches]
                                       [--out profiles/num_class_bench.json]"""
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
N, B, MODEL = 1024, 32, 'DGCNN'
SDA_C, SDA_M, SDA_HEADS = 40, 32, 3
WARMUP = 4
GROUPS = {'a': ('c10_parent', 'c10'), 'b': ('c40_composed', 'c40_fused'), 'c': ('sda_composed', 'sda_multi')}


def _stepper(arm):
    import torch
    import bench
    from oracle import ref_cpu as O
    from sug_amd import ops
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    C = 40 if arm.startswith('c40') else 10
    assert ops.HEADS_FUSED == (arm != 'c40_composed')
    torch.manual_seed(0)
    net = (Net_MDA(MODEL) if C == 10 else Net_MDA(MODEL, num_class=C)).cuda().train()      # (the parent tree has no num_class)
    g = torch.Generator().manual_seed(0)
    data, data_t = O.synth_clouds(B, N, g).cuda(), O.synth_clouds(B, N, g).cuda()
    label, label_t = torch.randint(0, C, (B,), generator=g).cuda(), torch.randint(0, C, (B,), generator=g).cuda()
    tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=True, methods=bench.BENCH_METHODS)

    def step():
        return tr.step(data, label, data_t, label_t)

    def end():
        if len(tr._graphs) != 1 or next(iter(tr._graphs.values()))['graph'] is None:
            raise RuntimeError('%s did not replay one graph' % arm)
    return step, end


def _sda(arm):
    import torch
    from sug_amd import ops
    from sug_amd.model import mmd
    from sug_amd.utils.common_utils import create_one_hot_labels
    g = torch.Generator().manual_seed(0)
    heads = [(torch.randn(SDA_M, SDA_C, generator=g).cuda() * 2, torch.randn(SDA_M, SDA_C, generator=g).cuda() * 2)
             for _ in range(SDA_HEADS)]
    ls, lt = torch.randint(0, SDA_C, (SDA_M,), generator=g).cuda(), torch.randint(0, SDA_C, (SDA_M,), generator=g).cuda()

    def composed_one(ps, pt):
        a = torch.cat((torch.softmax(ps, dim=1).view(-1, SDA_C), create_one_hot_labels(ls, SDA_C) * 0.5), dim=1)
        b = torch.cat((torch.softmax(pt, dim=1).view(-1, SDA_C), create_one_hot_labels(lt, SDA_C) * 0.5), dim=1)
        a, b = mmd.normalized(a), mmd.normalized(b)
        distance = (mmd._kl_div(a, b) * 0.5 + mmd._kl_div(b, a) * 0.5).sum(1)
        return mmd.distance2weights(distances=distance, method='mean2one')
    if arm == 'sda_multi':
        step = lambda: ops.sda_prob_weights_multi(heads, ls, lt, 0.5, 'mean2one')
    else:
        step = lambda: [composed_one(ps, pt) for ps, pt in heads]
    want, got = [composed_one(ps, pt) for ps, pt in heads], ops.sda_prob_weights_multi(heads, ls, lt, 0.5, 'mean2one')
    for w, o in zip(want, got):
        torch.testing.assert_close(o, w, rtol=2e-4, atol=1e-7)
    return step, lambda: None


def _make(arm):
    return _sda(arm) if arm.startswith('sda') else _stepper(arm)


def child_time(arm, windows, window_s):
    import torch
    step, end = _make(arm)
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
    return {'ms': ms, 'steps_per_window': n}


def child_steps(arm, steps):
    """`steps` steps after the warm-up (run under rocprofv3 by the parent process)."""
    import torch
    step, end = _make(arm)
    for _ in range(WARMUP + steps):
        step()
    end()
    torch.cuda.synchronize()
    return {}


def _env(arm):
    env = dict(os.environ)
    env['SUG_HEADS_FUSED'] = '0' if arm == 'c40_composed' else '1'
    return env


def _cmd(arm, parent, rest):
    """The child's command line; c10_parent runs this file's child against the tree `parent` (its sug_amd, bench, oracle)."""
    return [sys.executable, os.path.abspath(__file__), '--child', rest[0], '--arm', arm,
            '--tree', parent if arm == 'c10_parent' else HERE] + rest[1:]


def _child(arm, parent, rest, limit):
    r = subprocess.run(_cmd(arm, parent, rest), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, env=_env(arm))
    if r.returncode != 0:
        raise RuntimeError('child %s %s ended with %d:\n%s' % (arm, rest, r.returncode, r.stderr.decode()[-3000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _launches(arm, parent, steps, limit):
    """Kernel dispatches of a run of WARMUP + `steps` steps (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='num_class_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--'] + \
            _cmd(arm, parent, ['steps', '--steps', str(steps)])
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
    ap.add_argument('--parent', help='a built checkout of the parent commit: adds the arm c10_parent to group (a)')
    ap.add_argument('--groups', default='a,b,c')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--windows', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--child', choices=('time', 'steps'))
    ap.add_argument('--arm')
    ap.add_argument('--tree', default=HERE)
    ap.add_argument('--steps', type=int, default=2)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.abspath(a.tree))
        os.chdir(os.path.abspath(a.tree))
        fn = {'time': lambda: child_time(a.arm, a.windows, a.window), 'steps': lambda: child_steps(a.arm, a.steps)}[a.child]
        print(json.dumps(fn()))
        return
    parent = os.path.abspath(a.parent) if a.parent else None
    res = {'workload': 'SUGStep graph replay, %s %d per domain, N = %d, bench.BENCH_METHODS; SDA weights of %d heads, C = %d, m = %d'
                       % (MODEL, B, N, SDA_HEADS, SDA_C, SDA_M), 'dtype': 'fp32',
           'arms': {'c10': 'ten classes, this tree', 'c10_parent': 'ten classes, the parent commit',
                    'c40_fused': '40 classes, fused heads (64-wide backward instantiation)',
                    'c40_composed': '40 classes, SUG_HEADS_FUSED=0 (library head)',
                    'sda_multi': 'ops.sda_prob_weights_multi, one launch', 'sda_composed': 'torch ops, three heads in turn'},
           'units': {'a': 'ms per step', 'b': 'ms per step', 'c': 'ms per call of all three heads'},
           'rounds': a.rounds, 'windows_per_round': a.windows, 'window_s': a.window, 'results': []}
    failed = None
    for grp in a.groups.split(','):
        if failed is not None:                              # a child that failed may have faulted the GPU: start nothing more
            break
        arms = [arm for arm in GROUPS[grp] if arm != 'c10_parent' or parent]
        row = {'group': grp}
        try:
            ms = {arm: [] for arm in arms}
            for _ in range(a.rounds):
                for arm in arms:                            # the arms alternate within a round
                    r = _child(arm, parent, ['time', '--windows', str(a.windows), '--window', str(a.window)], 300)
                    ms[arm].append(r['ms'])
            for arm in arms:
                flat = [v for w in ms[arm] for v in w]
                med = statistics.median(flat)
                per_round = [statistics.median(w) for w in ms[arm]]
                row['ms_' + arm] = round(med, 5)
                row['spread_between_rounds_' + arm] = round((max(per_round) - min(per_round)) / med, 4)
                row['round_medians_ms_' + arm] = [round(v, 5) for v in per_round]
            if a.launches:
                for arm in arms:
                    lo, hi = (_launches(arm, parent, s, 300) for s in (2, 6))
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
