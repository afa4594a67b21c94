#!/usr/bin/env python3
"""PointTransformerCls (train_source.py, Model PTran) on one GPU.  Prints one JSON line:

  * ms per source-only train step (forward, CE, backward, one torch.optim.Adam step) at B = 32, N = 1024, fp32, with the
    fused head (sug_ptcls_head_*) and with the composed library head (SUG_PTCLS_HEAD_FUSED=0), and ms of the head alone
    (forward + backward on the last level's points);
  * kernel launches per step, from `rocprofv3 --kernel-trace --stats` runs of 2 and 6 steps (the difference over 4);
  * ms per eval_worker call (source_flag) over synthetic batches, against the eager loop it replaces.

Every measurement runs in a child process under its own time limit; the parent does not touch the GPU.
Usage: python tools/bench_ptran_cls.py [--steps 20] [--warmup 5] [--no-launches] [--out FILE]"""
import argparse
import copy
import csv
import glob
import json
import logging
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N = 32, 1024


def _setup():
    import torch
    from oracle import ref_cpu as O
    from sug_amd.model.Ptran_model import PointTransformerCls
    torch.manual_seed(0)
    net = PointTransformerCls().cuda().train()
    g = torch.Generator().manual_seed(0)
    x = O.synth_clouds(B, N, g).cuda()
    lab = torch.randint(0, 10, (B,), generator=g).cuda()
    return net, x, lab


def _timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def child_train(steps, warmup):
    import torch
    from sug_amd.model.Ptran_model import classify
    net, x, lab = _setup()
    opt = torch.optim.Adam(net.parameters(), lr=5e-4, weight_decay=1e-4)

    def step():
        loss = torch.nn.functional.cross_entropy(net(x), lab)
        opt.zero_grad()
        loss.backward()
        opt.step()

    res = {'step_ms': _timed(step, steps, warmup)}
    with torch.no_grad():
        points, _ = net.backbone(x)
    points = points.detach().requires_grad_(True)

    def head():
        classify(net.fc2, points).sum().backward()

    res['head_ms'] = _timed(head, steps * 10, warmup)
    return res


def child_eval(steps, warmup):
    import torch
    from oracle import ref_cpu as O
    from sug_amd.utils.eval_utils import eval_worker
    net, _, _ = _setup()
    net.eval()
    g = torch.Generator().manual_seed(1)
    batches = [(O.synth_clouds(B, N, g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()) for _ in range(8)]
    ce = torch.nn.CrossEntropyLoss().cuda()
    log = logging.getLogger('bench_ptran_cls')
    d = {'model': net, 'dataloader': batches, 'dataset': 'synthetic', 'best_target_acc': 0.0, 'device': torch.device('cuda:0'),
         'criterion': ce, 'epoch': 0, 'best_target_acc_epoch': 0, 'dataset_name': 'synthetic', 'num_class': 10,
         'cls_eval': False, 'source_flag': True}

    def worker():
        with torch.no_grad():
            eval_worker(dict(d), log)

    def eager():                 # the reference loop's device work: eval forward, CE, argmax, counts per batch
        hits, loss_sum = 0, 0.0
        with torch.no_grad():
            m = copy.deepcopy(net)
            for data, label in batches:
                y = m(data)
                loss_sum += ce(y, label).item() * data.shape[0]
                hits = hits + torch.sum(torch.max(y, 1)[1] == label)
        return hits, loss_sum

    ms_w = _timed(worker, steps, warmup)
    ms_e = _timed(eager, steps, warmup)
    return {'eval_worker_ms': ms_w, 'eval_eager_ms': ms_e, 'eval_batches': len(batches)}


def child_steps(steps):
    """`steps` train steps after 2 warm-up steps (run under rocprofv3 by the parent)."""
    import torch
    net, x, lab = _setup()
    opt = torch.optim.Adam(net.parameters(), lr=5e-4, weight_decay=1e-4)
    for _ in range(2 + steps):
        loss = torch.nn.functional.cross_entropy(net(x), lab)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return {}


def _child(args, env_extra, limit):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError('child %s ended with %d:\n%s' % (args, r.returncode, r.stderr.decode()[-3000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _launches(fused, steps, limit):
    """Kernel dispatches of a run of `steps` train steps (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='ptcls_prof_')
    try:
        env = dict(os.environ, SUG_PTCLS_HEAD_FUSED='1' if fused else '0')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--child', 'steps', '--steps', str(steps)]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
        if r.returncode != 0:
            raise RuntimeError('rocprofv3 run ended with %d:\n%s' % (r.returncode, r.stderr.decode()[-3000:]))
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if len(files) != 1:
            raise RuntimeError('expected one kernel_stats.csv, found %s' % files)
        rows = list(csv.DictReader(open(files[0])))
        key = lambda row, *names: next(row[c] for c in row if c.strip().lower() in names)
        return {key(row, 'name', 'kernel_name', 'kernel'): int(key(row, 'calls', 'count')) for row in rows}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--child', choices=('train', 'eval', 'steps'))
    ap.add_argument('--no-launches', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.child:
        fn = {'train': lambda: child_train(a.steps, a.warmup), 'eval': lambda: child_eval(a.steps, a.warmup),
              'steps': lambda: child_steps(a.steps)}[a.child]
        print(json.dumps(fn()))
        return
    res = {'workload': 'PointTransformerCls source-only train step', 'B': B, 'N': N, 'dtype': 'fp32'}
    common = ['--steps', str(a.steps), '--warmup', str(a.warmup)]
    for fused in (True, False):
        r = _child(['--child', 'train'] + common, {'SUG_PTCLS_HEAD_FUSED': '1' if fused else '0'}, 300)
        tag = 'fused' if fused else 'composed'
        res['step_ms_%s_head' % tag] = round(r['step_ms'], 3)
        res['head_fwd_bwd_ms_%s' % tag] = round(r['head_ms'], 4)
    res['step_saved_ms'] = round(res['step_ms_composed_head'] - res['step_ms_fused_head'], 3)
    if not a.no_launches:
        for fused in (True, False):
            try:
                lo, hi = _launches(fused, 2, 300), _launches(fused, 6, 300)
            except (RuntimeError, StopIteration, subprocess.TimeoutExpired) as e:
                res['launches_error'] = str(e)[-500:]
                break
            per = {k: (hi.get(k, 0) - lo.get(k, 0)) / 4 for k in set(lo) | set(hi)}
            tag = 'fused' if fused else 'composed'
            res['launches_per_step_%s_head' % tag] = round(sum(per.values()), 2)
            if fused:
                res['head_kernels_per_step'] = {k: v for k, v in sorted(per.items()) if 'ptcls' in k}
    r = _child(['--child', 'eval', '--steps', '5', '--warmup', '2'], {}, 300)
    res.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()})
    res['eval_speedup'] = round(res['eval_eager_ms'] / res['eval_worker_ms'], 2)
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
