#!/usr/bin/env python3
"""The classification-loss tail of the shipped configurations (CLS_LOSS ClassWeighting / FocalLoss, TARGET_LOSS 1.0) on one GPU:
what the fused tail (ops.cls_loss) saves over composing it from torch ops.  Prints one JSON line.

Workloads (DGCNN, 32 clouds per domain, N = 1024: BASELINE configuration 2; alpha on the device in every arm):
  sug     SUGStep(use_graph=True), benchmark METHODS + TARGET_LOSS 1.0, focal_loss(gamma=0, alpha=<DLSA-style class weights>)
  uda     UDAStep('naive_mmd', target_loss=1.0, use_graph=True), focal_loss(gamma=2)
  sug_ce  SUGStep(use_graph=True), benchmark METHODS, nn.CrossEntropyLoss(): the headline path (launches only)
Arms:
  fused     this tree
  composed  this tree with the tail composed: SUG_FUSED_LOSS=0 for SUGStep; for UDAStep a subclass of focal_loss, which the step
            does not recognise (fused_loss=False would also unfuse the heads)
  parent    the tree given with --parent (a built checkout of the parent commit), the same calls
Method, as tools/bench_uda_step.py: a fresh child process per (workload, arm, round); the arms alternate within a round, the
rounds repeat.  A child warms its one key up (planned, captured and replayed before any clock starts), sizes a window to at least
`--window` seconds from a short probe, and times `--windows` device-synchronised windows with the profiler off.  Reported per
arm: the median ms per step over all windows of all rounds and the window-to-window spread (max - min) / median; the parent's
spread is the yardstick for "not slower".  Launches per replayed step (--launches; runs of their own): `rocprofv3 --kernel-trace
--stats` runs of 2 and 6 steps after the warm-up, the difference over 4; the same for the loss tail alone on fixed logits,
forward and backward (`tail_*`).  --errors: the largest loss and gradient error of ops.cls_loss against the formula in fp64 on
the CPU, next to that of the composed fp32 module, over the combinations of tests/test_gpu_cls_loss.py at M = 32, C = 10.
The parent process does not touch the GPU.

Usage: python tools/bench_cls_loss.py [--parent DIR] [--workloads sug,uda] [--rounds 2] [--windows 3] [--window 1.0]
                                      [--launches] [--errors] [--no-time] [--out profiles/cls_loss_bench.json]"""
import argparse
import csv
import glob
import itertools
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
WARMUP = 4
# DLSA-style weights: (1 / class count)^q normalised to mean 1 for a long-tailed ten-class set
COUNTS = [3000, 2200, 1500, 900, 600, 400, 250, 150, 90, 60]
Q = 0.5
ALPHA = [(1.0 / c) ** Q for c in COUNTS]
ALPHA = [a * len(ALPHA) / sum(ALPHA) for a in ALPHA]


def _criterion(kind, composed):
    import torch
    from sug_amd.model.model_utils import focal_loss
    if kind == 'ce':
        return torch.nn.CrossEntropyLoss()
    cls = focal_loss
    if composed:
        class unrecognised_focal_loss(focal_loss):          # the same arithmetic; the steps recognise the exact type only
            pass
        cls = unrecognised_focal_loss
    c = cls(alpha=list(ALPHA), gamma=0, num_classes=10) if kind == 'class_weighting' else cls(gamma=2, num_classes=10)
    c.alpha = c.alpha.cuda()
    return c


def _stepper(workload, arm):
    """(step(), end()) of a workload in the tree on sys.path."""
    import torch
    import bench
    from oracle import ref_cpu as O
    from sug_amd.model.Model import Net_MDA
    torch.manual_seed(0)
    net = Net_MDA(MODEL).cuda().train()
    g = torch.Generator().manual_seed(0)
    batch = (O.synth_clouds(B, N, g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda(),
             O.synth_clouds(B, N, g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda())
    if workload in ('sug', 'sug_ce'):
        from sug_amd.train_step import SUGStep
        methods = dict(bench.BENCH_METHODS)
        if workload == 'sug':
            methods['TARGET_LOSS'] = 1.0
        tr = SUGStep(net, lr=1e-3, weight_decay=5e-5, use_graph=True, methods=methods,
                     criterion=_criterion('ce' if workload == 'sug_ce' else 'class_weighting', False))

        def end():
            want = {'sug_ce': 'ce_pair', 'sug': 'cls_loss' if arm == 'fused' else 'composed'}[workload]
            if arm != 'parent' and tr.loss_form != want:
                raise RuntimeError('%s/%s ran the %s tail, not %s' % (workload, arm, tr.loss_form, want))
            if len(tr._graphs) != 1:
                raise RuntimeError('%s/%s did not replay one graph' % (workload, arm))
        return (lambda: tr.step(*batch)), end
    from sug_amd.uda_step import UDAStep
    tr = UDAStep(net, recipe='naive_mmd', target_loss=1.0, lr=1e-3, weight_decay=5e-5, use_graph=True,
                 criterion=_criterion('focal', arm == 'composed'))

    def end():
        tr.epoch_totals()
        if tr.stats['captured'] != 1 or tr.stats['refused']:
            raise RuntimeError('uda/%s did not replay: %s (%s)' % (arm, tr.stats, tr.why))
        if arm != 'parent' and tr.loss_form != ('cls_loss' if arm == 'fused' else 'composed'):
            raise RuntimeError('uda/%s ran the %s tail' % (arm, tr.loss_form))
    return (lambda: tr.step(*batch)), end


def _tail(workload, arm):
    """The loss tail alone on fixed logits [B, 10], forward and backward, with the workload's coefficients."""
    import torch
    from sug_amd import ops
    from sug_amd.train_step import discrepancy
    g = torch.Generator().manual_seed(0)
    zs = [(torch.randn(B, 10, generator=g) * 3).cuda().requires_grad_() for _ in range(4)]
    label = torch.randint(0, 10, (B,), generator=g).cuda()
    crit = _criterion('class_weighting' if workload == 'sug' else 'focal', False)
    a_s, a_t, a_d = (0.25, 0.25, 0.0) if workload == 'sug' else (0.25, 0.25, 1.0)
    gamma = 0.0 if workload == 'sug' else 2.0

    def step():
        if arm == 'tail_fused':
            loss = ops.cls_loss(zs[0], zs[1], zs[2], zs[3], label, label, crit.alpha, gamma, 'mean', -100, a_s, a_t, a_d)[0]
        elif workload == 'sug':                             # train_step.py: the composed block, TARGET_LOSS > 0, ADV_WEIGHT 0
            loss_s = 0.5 * (crit(zs[0], label) + crit(zs[1], label))
            loss_t = 0.5 * (crit(zs[2], label) + crit(zs[3], label))
            loss = 1.0 * (0.5 * (loss_s + loss_t))
        else:                                               # uda_step.py: the composed block, naive_mmd, TARGET_LOSS > 0
            loss_s = 0.5 * crit(zs[0], label) + 0.5 * crit(zs[1], label)
            loss_adv = - 1 * discrepancy(zs[2], zs[3])
            loss_t = 0.5 * crit(zs[2], label) + 0.5 * crit(zs[3], label)
            loss = 0.5 * 1.0 * loss_s + loss_adv + 0.5 * 1.0 * loss_t
        loss.backward()
        for z in zs:
            z.grad = None
    return step, lambda: None


def child_time(workload, arm, windows, window_s):
    import torch
    step, end = _stepper(workload, arm)
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


def child_steps(workload, arm, steps):
    """`steps` steps after the warm-up (run under rocprofv3 by the parent process)."""
    import torch
    step, end = _tail(workload, arm) if arm.startswith('tail_') else _stepper(workload, arm)
    for _ in range(WARMUP + steps):
        step()
    end()
    torch.cuda.synchronize()
    return {}


def child_errors():
    """Largest |error| of the four outputs (relative to max(1, |ref|)) and of the gradients (relative to the largest entry of the
    block) against the formula in fp64 on the CPU: ops.cls_loss, and the same formula composed from torch ops in fp32 on the GPU."""
    import torch
    import torch.nn.functional as F
    from sug_amd import ops

    def composed(zs, lab, alpha, gamma, reduction, a_s, a_t, a_d):
        def one(z):
            logp = F.log_softmax(z, dim=1).gather(1, lab.view(-1, 1)).view(-1)
            loss = alpha.gather(0, lab) * (-(1 - torch.exp(logp)) ** gamma * logp)
            return loss.mean() if reduction == 'mean' else loss.sum()
        Ls, Lt = one(zs[0]) + one(zs[1]), one(zs[2]) + one(zs[3])
        D = torch.mean(torch.abs(F.softmax(zs[2], dim=-1) - F.softmax(zs[3], dim=-1)))
        return a_s * Ls + a_t * Lt - a_d * D

    def run(fn, zs, dtype, device):
        zs = [z.to(device=device, dtype=dtype).requires_grad_() for z in zs]
        loss = fn(zs)
        (loss * 1.7).backward()
        return loss.detach().double().cpu(), [z.grad.double().cpu() for z in zs]
    worst = {'cls_loss': [0.0, 0.0], 'composed_fp32': [0.0, 0.0]}
    M, C = 32, 10
    for scale, seed in itertools.product((3.0, 12.0), (0, 1, 2)):
        g = torch.Generator().manual_seed(seed)
        zs = [torch.randn(M, C, generator=g) * scale for _ in range(4)]
        lab = torch.randint(0, C, (M,), generator=g)
        for gamma, per_class, reduction, (a_t, a_d) in itertools.product((0.0, 1.5, 2.0), (False, True), ('mean', 'sum'),
                                                                         ((0.25, 0.0), (0.25, 0.15))):
            alpha = torch.tensor(ALPHA) if per_class else torch.full((C,), 1.0 / C)
            ref, gref = run(lambda z: composed(z, lab, alpha.double(), gamma, reduction, 0.35, a_t, a_d), zs, torch.float64, 'cpu')
            arms = {'composed_fp32': lambda z: composed(z, lab.cuda(), alpha.cuda(), gamma, reduction, 0.35, a_t, a_d),
                    'cls_loss': lambda z: ops.cls_loss(z[0], z[1], z[2], z[3], lab.cuda(), lab.cuda(), alpha.cuda(), gamma, reduction, -100,
                                                       0.35, a_t, a_d)[0]}
            for name, fn in arms.items():
                got, ggot = run(fn, zs, torch.float32, 'cuda')
                worst[name][0] = max(worst[name][0], float((got - ref).abs() / ref.abs().clamp_min(1.0)))
                worst[name][1] = max(worst[name][1], max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ggot, gref)))
    return {k: {'loss': v[0], 'gradient_over_largest_entry': v[1]} for k, v in worst.items()}


def _child(root, args, limit, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--root', root] + args, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=limit, env=env)
    if r.returncode != 0:
        raise RuntimeError('child %s ended with %d:\n%s' % (args, r.returncode, r.stderr.decode()[-3000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _launches(root, workload, arm, steps, limit, env):
    """Kernel dispatches of a run of WARMUP + `steps` steps (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='cls_loss_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--root', root, '--child', 'steps', '--workload', workload, '--arm', arm,
               '--steps', str(steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, env=env)
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


def _env(arm):
    env = dict(os.environ)
    env['SUG_FUSED_LOSS'] = '0' if arm == 'composed' else '1'
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help='a built checkout of the parent commit (arm "parent")')
    ap.add_argument('--workloads', default='sug,uda')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--errors', action='store_true')
    ap.add_argument('--no-time', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--child', choices=('time', 'steps', 'errors'))
    ap.add_argument('--workload')
    ap.add_argument('--arm')
    ap.add_argument('--steps', type=int, default=2)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.abspath(a.root))         # the tree under test: this one, or the parent's
        fn = {'time': lambda: child_time(a.workload, a.arm, a.windows, a.window),
              'steps': lambda: child_steps(a.workload, a.arm, a.steps), 'errors': child_errors}[a.child]
        print(json.dumps(fn()))
        return
    arms = ['fused', 'composed'] + (['parent'] if a.parent else [])
    root = {'fused': HERE, 'composed': HERE, 'parent': os.path.abspath(a.parent) if a.parent else None}
    res = {'workload': 'classification-loss tail of the shipped configurations, %s %d per domain, N = %d' % (MODEL, B, N),
           'dtype': 'fp32', 'alpha': [round(v, 6) for v in ALPHA], 'arms': {
               'fused': 'this tree (ops.cls_loss)', 'composed': 'this tree, the tail composed from torch ops',
               'parent': 'the parent commit'}, 'rounds': a.rounds, 'windows_per_round': a.windows, 'window_s': a.window,
           'results': []}
    failed = None
    for workload in a.workloads.split(','):
        if failed is not None:                              # a child that failed may have faulted the GPU: start nothing more
            break
        row = {'workload': workload}
        try:
            if not a.no_time:
                ms = {arm: [] for arm in arms}
                for _ in range(a.rounds):
                    for arm in arms:                        # the arms alternate within a round
                        r = _child(root[arm], ['--child', 'time', '--workload', workload, '--arm', arm, '--windows', str(a.windows),
                                               '--window', str(a.window)], 600, _env(arm))
                        ms[arm] += r['ms']
                for arm in arms:
                    med = statistics.median(ms[arm])
                    row['ms_' + arm] = round(med, 4)
                    row['spread_' + arm] = round((max(ms[arm]) - min(ms[arm])) / med, 4)
                    row['windows_ms_' + arm] = [round(v, 4) for v in ms[arm]]
            if a.launches:
                for arm in arms:
                    lo, hi = (_launches(root[arm], workload, arm, s, 600, _env(arm)) for s in (2, 6))
                    row['launches_per_step_' + arm] = round((hi - lo) / 4, 2)
                for arm in ('tail_composed', 'tail_fused'):
                    lo, hi = (_launches(HERE, workload, arm, s, 600, _env('fused')) for s in (2, 6))
                    row['launches_' + arm] = round((hi - lo) / 4, 2)
        except (RuntimeError, StopIteration, subprocess.TimeoutExpired) as e:
            failed = row['error'] = str(e)[-800:]
        res['results'].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if a.launches and failed is None:                       # the headline path launches what it did
        row = {'workload': 'sug_ce'}
        try:
            for arm in ['fused'] + (['parent'] if a.parent else []):
                lo, hi = (_launches(root[arm], 'sug_ce', arm, s, 600, _env(arm)) for s in (2, 6))
                row['launches_per_step_' + arm] = round((hi - lo) / 4, 2)
        except (RuntimeError, StopIteration, subprocess.TimeoutExpired) as e:
            failed = row['error'] = str(e)[-800:]
        res['results'].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if a.errors and failed is None:
        try:
            res['errors_vs_fp64'] = _child(HERE, ['--child', 'errors'], 600)
        except (RuntimeError, subprocess.TimeoutExpired) as e:
            failed = res['errors_error'] = str(e)[-800:]
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)
    if failed is not None:
        sys.exit(1)


if __name__ == '__main__':
    main()
