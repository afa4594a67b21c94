#!/usr/bin/env python3
"""The two-phase UDA step (train_uda.py:149-184) on one GPU.  Prints one JSON line.

Arms, per backbone and batch size (rows per domain):
  a  the caller's literal loop: four model(...) calls, nn.CrossEntropyLoss and discrepancy from torch ops, two backwards, three
     sug_amd.optim.Adam, the three loss.item() reads and the running totals every step (nothing but the API the package had before
     UDAStep: runs unchanged on an older tree; Net_MDA's per-call graphs stay at their default);
  b  UDAStep(use_graph=False): the paired step with ops.mcd_loss and the device-resident totals, launched eagerly;
  c  UDAStep(use_graph=True): planned, captured, replayed.
Default size: DGCNN, 32 clouds per domain, N = 1024 (BASELINE configuration 2).

Method: a fresh child process per (backbone, arm, round); the arms alternate within a round, the rounds repeat.  A child warms
its one key up (the graph arm: planned, captured and replayed before any clock starts), sizes a window to at least `--window`
seconds from a short probe, and times `--windows` device-synchronised windows with the profiler off (arms b / c read
epoch_totals() once per window, inside it).  Reported per arm: the median ms per step over all windows of all rounds and the
window-to-window spread (max - min) / median.  Launches per step (--launches; runs of their own): `rocprofv3 --kernel-trace
--stats` runs of 2 and 6 steps after the warm-up, the difference over 4; the same for the phase-1 loss tail alone on fixed
logits, forward and backward, composed from torch ops (`tail_composed`) and as ops.mcd_loss (`tail_fused`).
The parent process does not touch the GPU.

Usage: python tools/bench_uda_step.py [--arms a,b,c] [--configs DGCNN:32,...] [--recipe uda] [--rounds 2] [--windows 3]
                                      [--window 1.0] [--launches] [--no-time] [--out FILE]"""
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
CONFIGS = [('DGCNN', 32)]
WARMUP = 4


def _setup(name, B):
    import torch
    from oracle import ref_cpu as O
    from sug_amd.model.Model import Net_MDA
    torch.manual_seed(0)
    net = Net_MDA(name).cuda().train()
    g = torch.Generator().manual_seed(0)
    batch = (O.synth_clouds(B, N, g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda(),
             O.synth_clouds(B, N, g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda())
    return net, batch


def _stepper(name, B, arm, recipe):
    """(step(), window_end()) of an arm."""
    import torch
    net, (data, label, data_t, label_t) = _setup(name, B)
    if arm == 'a':
        from sug_amd.model import mmd
        from sug_amd.optim import Adam
        from sug_amd.train_step import discrepancy
        model, lr, wd = net, 1e-3, 5e-5
        criterion = torch.nn.CrossEntropyLoss().cuda()
        params = [{'params': v} for k, v in model.g.named_parameters() if 'pred_offset' not in k]
        optimizer_g = Adam(params, lr=lr, weight_decay=wd)
        optimizer_c = Adam([{'params': model.c1.parameters()}, {'params': model.c2.parameters()}],
                           lr=lr * 2 if recipe == 'uda' else lr, weight_decay=wd)
        optimizer_dis = Adam([{'params': model.g.parameters()}, {'params': model.attention_s.parameters()},
                              {'params': model.attention_t.parameters()}], lr=lr, weight_decay=wd)
        class_mmd = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 1.0}
        tot = [0.0, 0.0, 0.0, 0, 0]

        def step():
            pred_s1, pred_s2 = model(data)
            pred_t1, pred_t2 = model(data_t, constant=1.0, adaptation=True)
            loss_s1 = criterion(pred_s1, label)
            loss_s2 = criterion(pred_s2, label)
            loss_adv = - 1 * discrepancy(pred_t1, pred_t2)
            if recipe == 'uda':
                loss_s = loss_s1 + loss_s2
            else:
                loss_s = 0.5 * loss_s1 + 0.5 * loss_s2
            loss = loss_s + loss_adv
            loss.backward()
            optimizer_g.step()
            optimizer_c.step()
            optimizer_g.zero_grad()
            optimizer_c.zero_grad()
            feat_node_s = model(data, node_adaptation_s=True)
            feat_node_t = model(data_t, node_adaptation_t=True)
            if recipe == 'uda':
                loss_node_adv = 1 * mmd.mix_rbf_mmd2(feat_node_s, feat_node_t, [0.01, 0.1, 1, 10, 100])
            else:
                loss_node_adv = 1 * mmd.mmd_cal(label, feat_node_s, label_t, feat_node_t, class_mmd)
            loss = loss_node_adv
            loss.backward()
            optimizer_dis.step()
            optimizer_dis.zero_grad()
            tot[0] += loss_s.item() * data.size(0)
            tot[1] += loss_adv.item() * data.size(0)
            tot[2] += loss_node_adv.item() * data.size(0)
            tot[3] += data.size(0)
            tot[4] += data_t.size(0)
        return step, lambda: None
    from sug_amd.uda_step import UDAStep
    tr = UDAStep(net, recipe=recipe, lr=1e-3, weight_decay=5e-5, use_graph=(arm == 'c'))

    def end():
        tr.epoch_totals()
        if arm == 'c' and (tr.stats['captured'] != 1 or tr.stats['refused']):
            raise RuntimeError('arm c did not replay: %s (%s)' % (tr.stats, tr.why))
    return (lambda: tr.step(data, label, data_t, label_t)), end


def _tail(B, arm):
    """The phase-1 loss tail alone on fixed logits [B, 10], forward and backward."""
    import torch
    from sug_amd import ops
    from sug_amd.train_step import discrepancy
    g = torch.Generator().manual_seed(0)
    zs = [(torch.randn(B, 10, generator=g) * 3).cuda().requires_grad_() for _ in range(4)]
    label = torch.randint(0, 10, (B,), generator=g).cuda()
    criterion = torch.nn.CrossEntropyLoss().cuda()

    def step():
        if arm == 'tail_fused':
            loss = ops.mcd_loss(zs[0], zs[1], zs[2], zs[3], label)[0]
        else:
            loss_s = criterion(zs[0], label) + criterion(zs[1], label)
            loss = 1.0 * loss_s + (- 1 * discrepancy(zs[2], zs[3]))
        loss.backward()
        for z in zs:
            z.grad = None
    return step, lambda: None


def child_time(name, B, arm, recipe, windows, window_s):
    import torch
    step, end = _stepper(name, B, arm, recipe)
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


def child_steps(name, B, arm, recipe, steps):
    """`steps` steps after the warm-up (run under rocprofv3 by the parent)."""
    import torch
    step, end = _tail(B, arm) if arm.startswith('tail_') else _stepper(name, B, arm, recipe)
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


def _launches(name, B, arm, recipe, steps, limit):
    """Kernel dispatches of a run of WARMUP + `steps` steps (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='uda_step_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--child', 'steps', '--model', name, '--B', str(B), '--arm', arm,
               '--recipe', recipe, '--steps', str(steps)]
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
    ap.add_argument('--recipe', default='uda', choices=('uda', 'naive_mmd'))
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
        fn = {'time': lambda: child_time(a.model, a.B, a.arm, a.recipe, a.windows, a.window),
              'steps': lambda: child_steps(a.model, a.B, a.arm, a.recipe, a.steps)}[a.child]
        print(json.dumps(fn()))
        return
    arms = a.arms.split(',')
    configs = [(c.split(':')[0], int(c.split(':')[1])) for c in a.configs.split(',')]
    res = {'workload': 'two-phase UDA train step (train_uda.py:149-184), recipe %s' % a.recipe, 'N': N, 'dtype': 'fp32', 'arms': {
        'a': 'caller\'s literal loop: four model(...) calls, three sug_amd.optim.Adam, three loss.item() every step',
        'b': 'UDAStep(use_graph=False)', 'c': 'UDAStep(use_graph=True)'}, 'rounds': a.rounds, 'windows_per_round': a.windows,
        'window_s': a.window, 'results': []}
    failed = None
    for name, B in configs:
        if failed is not None:                              # a child that failed may have faulted the GPU: start nothing more
            break
        row = {'model': name, 'B': B}
        if not a.no_time:
            ms = {arm: [] for arm in arms}
            for _ in range(a.rounds):
                for arm in arms:                            # the arms alternate within a round
                    r = _child(['--child', 'time', '--model', name, '--B', str(B), '--arm', arm, '--recipe', a.recipe,
                                '--windows', str(a.windows), '--window', str(a.window)], 600)
                    ms[arm] += r['ms']
            for arm in arms:
                med = statistics.median(ms[arm])
                row['ms_' + arm] = round(med, 4)
                row['spread_' + arm] = round((max(ms[arm]) - min(ms[arm])) / med, 4)
                row['windows_ms_' + arm] = [round(v, 4) for v in ms[arm]]
            if 'a' in arms and 'c' in arms:
                row['speedup_c_over_a'] = round(row['ms_a'] / row['ms_c'], 3)
        if a.launches:
            for arm in arms + ['tail_composed', 'tail_fused']:
                try:
                    lo, hi = _launches(name, B, arm, a.recipe, 2, 600), _launches(name, B, arm, a.recipe, 6, 600)
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
