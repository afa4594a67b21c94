"""Milliseconds per eval_worker call (utils/eval_utils.py) on a synthetic test set, two forms alternated in one process:

  (a) the reference's evaluation loop, restated here, over sug_amd's eager eval-mode forward (model(data) kernel by kernel,
      metrics with per-class boolean masks and a host read each);
  (b) sug_amd.utils.eval_utils.eval_worker (graph-replayed forward, one sug_eval_accumulate launch per batch, one host
      synchronisation per call).

Each call gets a fresh copy.deepcopy of the model, as train_dg_single_gpu.py:364 hands one over; 80 full batches plus one
partial batch; one warm call of each form first.  Prints one JSON line per model.  --form b --calls 1 under
`rocprofv3 --kernel-trace --stats` (a separate run) gives the kernels' time per batch, the floor of either form.

usage: python tools/bench_eval.py [--models DGCNN,Pointnet,Pointnet2,PTran] [--batches 80] [--reps 3] [--form ab]
"""
import argparse
import copy
import json
import logging
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {'DGCNN': (32, 1024), 'Pointnet': (8, 1024), 'Pointnet2': (64, 2048), 'PTran': (16, 2048)}


def synth(B, N, gen):
    """bench.py's clouds: U(-1,1)^3 -> centred, unit sphere; labels randint(0, 10)."""
    pc = torch.rand(B, N, 3, generator=gen) * 2 - 1
    pc = pc - pc.mean(dim=1, keepdim=True)
    pc = pc / pc.pow(2).sum(-1).sqrt().max(dim=1)[0].view(B, 1, 1)
    return pc.permute(0, 2, 1).unsqueeze(-1).contiguous(), torch.randint(0, 10, (B,), generator=gen)


class _Counter:
    n = 0


def reference_loop(model, loader, criterion, num_class, sync):
    """(a): the reference loop's arithmetic and host reads, cls_eval on; sync.n counts the host waits."""
    acc = np.zeros((num_class, 3))
    ratios, loss_sum, n_rows, hits = [], 0.0, 0, 0
    for data, label in loader:
        y1, y2 = model(data)
        output = (y1 + y2) / 2
        loss = criterion(output, label)
        pred = torch.max(output, 1)[1]
        classes = np.unique(label.cpu())                       # 1 wait
        sync.n += 1
        for c in classes:
            sel = label == int(c)
            k = pred[sel].eq(label[sel]).cpu().sum()           # two boolean-mask gathers + .cpu(): 3 waits
            acc[c, 0] += k.item() / float(data[sel].size(0))  # a third mask: 1 wait
            acc[c, 1] += 1
            sync.n += 4
        ratios.append(pred.eq(label).cpu().sum().item() / float(data.size(0)))
        loss_sum += loss.item() * data.size(0)                # 2 waits
        sync.n += 2
        hits = hits + torch.sum(pred == label)
        n_rows += data.size(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        acc[:, 2] = acc[:, 0] / acc[:, 1]
    return hits.double() / n_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='DGCNN,Pointnet,Pointnet2,PTran')
    ap.add_argument('--batches', type=int, default=80)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--form', default='ab', help='a, b or ab')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    from oracle import ref_cpu as O
    from sug_amd.model.Model import Net_MDA
    from sug_amd.utils import eval_utils
    dev = torch.device('cuda:0')
    log = logging.getLogger('bench_eval')
    log.addHandler(logging.NullHandler())
    log.propagate = False
    ce = nn.CrossEntropyLoss().to(dev)
    for name in args.models.split(','):
        B, N = SIZES[name]
        g = torch.Generator().manual_seed(666)
        torch.manual_seed(666)
        net = Net_MDA(name)
        net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 1))
        net = net.to(dev).train()
        with torch.no_grad():
            net(synth(B, N, g)[0].to(dev))                     # BatchNorm running buffers
        net.eval()
        loader = [tuple(t.to(dev) for t in synth(b, N, g)) for b in [B] * args.batches + [B // 2]]
        clouds = sum(d.shape[0] for d, _ in loader)
        times = {'a': [], 'b': []}
        syncs = {}

        def run(form):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                m = copy.deepcopy(net)
                if form == 'a':
                    c = _Counter()
                    reference_loop(m, loader, ce, 10, c)
                    torch.cuda.synchronize()
                    s = c.n
                else:
                    d = {'model': m, 'dataloader': loader, 'dataset': 'test', 'best_target_acc': 0.0, 'device': dev,
                         'criterion': ce, 'epoch': 0, 'best_target_acc_epoch': 0, 'dataset_name': 'synthetic',
                         'num_class': 10, 'cls_eval': True}
                    eval_utils.eval_worker(d, log)
                    torch.cuda.synchronize()
                    s = eval_utils.LAST['syncs']
            return (time.perf_counter() - t0) * 1e3, s

        forms = [f for f in 'ab' if f in args.form]
        for f in forms:                                         # warm call (form b: the keys' eager + capture calls)
            run(f)
        if 'b' in forms:
            run('b')
        for _ in range(args.reps):
            for f in forms:
                ms, s = run(f)
                times[f].append(ms)
                syncs[f] = s
        res = {'model': name, 'batch': B, 'npoints': N, 'batches_per_call': len(loader), 'clouds_per_call': clouds,
               'reps': args.reps}
        for f in forms:
            ms = float(np.median(times[f]))
            res['ms_per_call_' + f] = round(ms, 2)
            res['ms_all_' + f] = [round(t, 2) for t in times[f]]
            res['clouds_per_s_' + f] = round(clouds / ms * 1e3, 1)
            res['syncs_per_batch_' + f] = round(syncs[f] / len(loader), 3)
            res['syncs_per_call_' + f] = syncs[f]
        if 'b' in forms:
            res['eval_worker_form'] = eval_utils.LAST['form']
            res['graph_stats'] = eval_utils.LAST['stats']
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
