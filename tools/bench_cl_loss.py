#!/usr/bin/env python3
"""The contrastive alignment mode (NAME: CL) on one GPU, at the op level and in the training step.  Prints one JSON line.

The parent commit cannot run this mode at all (mmd_cal raised for the name), so the baseline of every figure is the COMPOSED
arm of this same tree: the composed lines of mmd.contrastive_loss_weighted (nn.CosineEmbeddingLoss and torch ops on the same
device tensors), selected with SUG_CL_LOSS=0 in the child's environment (the knob is read at import).

Op level: forward + backward of mmd.cl_loss_multi on three terms of one batch -- D = 4096 (node features), 256, 256 (the two
semantic heads), margins 0.2, no sample weights -- at m = 32 and m = 64 rows per domain.  Inputs: x = randn, y = 0.5 x + randn,
labels randint(0, 10), seeded.
Step level: SUGStep, DGCNN, 32 clouds per domain, N = 1024, bench.py's synthetic batch, GEO_MMD and SEM_MMD both NAME: CL
with the SDA weights of the shipped configuration (mean2one on both levels): replayed (use_graph=True), eager
(use_graph=False), and the composed arm eager; the same step with SOFT_MMD, replayed and eager, as context.
Method: every arm is a child process of its own (the parent does not touch the GPU); the arms alternate within a round,
`--rounds` rounds, each child timing `--windows` windows of at least `--window` seconds (sized from a short probe after the
warm-up) that end in a device synchronise, profiler off.  Per arm: median ms per call over all windows, and the spread
(max - min) / median between the rounds' medians.  Launches per call (--launches, runs of their own): kernel dispatches of
`rocprofv3 --kernel-trace --stats` runs of 2 and 6 calls after the warm-up, the difference over 4.

Usage: python tools/bench_cl_loss.py [--rounds 3] [--windows 2] [--window 0.3] [--launches] [--out profiles/cl_loss_bench.json]"""
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
OP_SHAPES = (32, 64)
OP_DIMS = (4096, 256, 256)
OP_ARMS = ('composed', 'fused')
STEP_ARMS = ('cl_composed_eager', 'cl_eager', 'cl_replayed', 'soft_eager', 'soft_replayed')
STEP_B, STEP_N = 32, 1024
WARMUP = 5


def _env(arm):
    env = dict(os.environ)
    env['SUG_CL_LOSS'] = '0' if 'composed' in arm else '1'
    return env


def _op_caller(m):
    import torch
    from sug_amd.model import mmd
    g = torch.Generator().manual_seed(m)
    ls, lt = torch.randint(0, 10, (m,), generator=g).cuda(), torch.randint(0, 10, (m,), generator=g).cuda()
    terms, leaves = [], []
    for D in OP_DIMS:
        X = torch.randn(m, D, generator=g)
        Y = 0.5 * X + torch.randn(m, D, generator=g)
        X, Y = X.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)
        leaves += [X, Y]
        terms.append((X, Y, {'NAME': 'CL', 'MARGIN': 0.2}, None, None))

    def call():
        for t in leaves:
            t.grad = None
        v = mmd.cl_loss_multi(ls, lt, terms)
        (v[0] + v[1] + v[2]).backward()
    return call


def _step_caller(arm):
    import torch
    import bench
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    if arm.startswith('cl_'):
        methods = {'GEO_MMD': [{'NAME': 'CL', 'MARGIN': 0.2, 'GEO_WEIGHTS': 'mean2one', 'GEO_SCALE': 1}],
                   'SEM_MMD': [{'NAME': 'CL', 'MARGIN': 0.2, 'SEM_WEIGHTS': 'mean2one', 'LABEL_WEIGHT': 0.5, 'SEM_SCALE': 1}]}
    else:
        methods = bench.BENCH_METHODS
    torch.manual_seed(0)
    model = Net_MDA('DGCNN').cuda().train()
    tr = SUGStep(model, lr=1e-3, weight_decay=5e-5, use_graph=arm.endswith('replayed'), methods=methods)
    batch = bench.synth(STEP_B, STEP_N, 666, 'cuda')
    return lambda: tr.step(*batch)


def _time(calls, windows, window_s):
    import torch
    out = {}
    for key, call in calls.items():
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        k = max(10, int(window_s / ((time.perf_counter() - t) / 10) * 1.1) + 1)
        w = []
        for _ in range(windows):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(k):
                call()
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t) / k * 1e3)
        out[key] = {'ms': w, 'calls_per_window': k}
    return out


def _callers(level, arm):
    return {str(m): _op_caller(m) for m in OP_SHAPES} if level == 'op' else {'step': _step_caller(arm)}


def child_calls(level, arm, key, count):
    """`count` calls after the warm-up (run under rocprofv3 by the parent process)."""
    import torch
    call = _op_caller(int(key)) if level == 'op' else _step_caller(arm)
    for _ in range(WARMUP + count):
        call()
    torch.cuda.synchronize()
    return {}


def _child(args, arm, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=limit, env=_env(arm))
    if r.returncode != 0:
        raise RuntimeError('child %s ended with %d:\n%s' % (args, r.returncode, r.stderr.decode()[-3000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _launches(level, arm, key, count, limit):
    """Kernel dispatches of a run of WARMUP + `count` calls (rocprofv3 --kernel-trace --stats)."""
    print('launches %s / %s / %s calls' % (level, arm, count), file=sys.stderr, flush=True)
    tmp = tempfile.mkdtemp(prefix='cl_loss_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--child', 'calls', '--level', level, '--arm', arm, '--key', key,
               '--count', str(count)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, env=_env(arm))
        if r.returncode != 0:
            raise RuntimeError('rocprofv3 run ended with %d:\n%s' % (r.returncode, r.stderr.decode()[-3000:]))
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if len(files) != 1:
            raise RuntimeError('expected one kernel_stats.csv, found %s' % files)
        rows = list(csv.DictReader(open(files[0])))
        key_of = lambda row, *names: next(row[c] for c in row if c.strip().lower() in names)
        return sum(int(key_of(row, 'calls', 'count')) for row in rows)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _summary(per_round):
    """per_round: [[ms of a window, ...] per round] -> the figures of one arm."""
    flat = [v for w in per_round for v in w]
    med = statistics.median(flat)
    meds = [statistics.median(w) for w in per_round]
    return {'ms': round(med, 4), 'spread_between_rounds': round((max(meds) - min(meds)) / med, 4),
            'round_medians_ms': [round(v, 4) for v in meds]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--windows', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--child', choices=('time', 'calls'))
    ap.add_argument('--level', choices=('op', 'step'))
    ap.add_argument('--arm')
    ap.add_argument('--key')
    ap.add_argument('--count', type=int, default=2)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, HERE)
        if a.child == 'time':
            print(json.dumps(_time(_callers(a.level, a.arm), a.windows, a.window)))
        else:
            print(json.dumps(child_calls(a.level, a.arm, a.key, a.count)))
        return
    res = {'baseline': 'the composed arm of this tree: the parent commit raises for NAME: CL, there is nothing older to compare with',
           'dtype': 'fp32',
           'op_workload': 'forward + backward of mmd.cl_loss_multi, three terms D = %s, margin 0.2, no sample weights' % (OP_DIMS,),
           'step_workload': 'SUGStep.step, DGCNN, %d clouds per domain, N = %d, synthetic batch of bench.py, SDA weights mean2one on '
                            'both levels' % (STEP_B, STEP_N),
           'arms': {'composed': 'SUG_CL_LOSS=0: nn.CosineEmbeddingLoss + torch ops, term by term (eager)',
                    'fused': 'ops.cl_loss_multi (sug_cl_loss_fwd / _bwd), eager launches',
                    'cl_composed_eager': 'NAME: CL, SUG_CL_LOSS=0, use_graph=False', 'cl_eager': 'NAME: CL, use_graph=False',
                    'cl_replayed': 'NAME: CL, use_graph=True', 'soft_eager': 'SOFT_MMD (context), use_graph=False',
                    'soft_replayed': 'SOFT_MMD (context), use_graph=True'},
           'rounds': a.rounds, 'windows_per_round': a.windows, 'window_s': a.window, 'op': [], 'step': {}}
    failed = None
    try:
        timed = {}
        targs = ['--child', 'time', '--windows', str(a.windows), '--window', str(a.window)]
        for _ in range(a.rounds):                           # the arms alternate within a round
            for level, arms in (('op', OP_ARMS), ('step', STEP_ARMS)):
                for arm in arms:
                    print('timing %s / %s' % (level, arm), file=sys.stderr, flush=True)
                    for key, r in _child(targs + ['--level', level, '--arm', arm], arm, 600).items():
                        slot = timed.setdefault((level, arm, key), {'ms': [], 'calls_per_window': r['calls_per_window']})
                        slot['ms'].append(r['ms'])
        for m in OP_SHAPES:
            row = {'m': m, 'D': list(OP_DIMS)}
            for arm in OP_ARMS:
                row[arm] = dict(_summary(timed[('op', arm, str(m))]['ms']), calls_per_window=timed[('op', arm, str(m))]['calls_per_window'])
            res['op'].append(row)
        for arm in STEP_ARMS:
            res['step'][arm] = dict(_summary(timed[('step', arm, 'step')]['ms']),
                                    calls_per_window=timed[('step', arm, 'step')]['calls_per_window'])
        if a.launches:                                      # (a child that fails may have faulted the GPU: the except ends it all)
            for row in res['op']:
                for arm in OP_ARMS:
                    lo, hi = (_launches('op', arm, str(row['m']), c, 300) for c in (2, 6))
                    row[arm]['launches_per_call'] = round((hi - lo) / 4, 2)
            for arm in STEP_ARMS:
                lo, hi = (_launches('step', arm, 'step', c, 300) for c in (2, 6))
                res['step'][arm]['launches_per_call'] = round((hi - lo) / 4, 2)
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
