#!/usr/bin/env python3
"""Device-resident data pipeline: what DeviceLoader costs, alone and in front of the headline step, and what the host
path it replaces delivers.

    python tools/bench_data_pipeline.py [--epochs 5] [--steps 100] [--out profiles/data_pipeline_bench.json]
    python tools/bench_data_pipeline.py --host-baseline      # (c) alone; the full run starts it as a child process

(a) DeviceLoader over M = 4096 synthetic clouds of P = 2048 points, aug on, at the config-2 shape (N = 1024, batch 32,
    pre-rotation on: a random subset per cloud) and the config-3 shape (N = 2048, batch 64): microseconds per batch and
    clouds/s over whole epochs (host clock around epochs that end in a device synchronise), and the kernel alone (device
    events around back-to-back launches into a fixed buffer) with its algorithmic bytes 12 B (P + N) over that time.
(b) The headline step (DGCNN, 32 + 32 clouds of 1024 points, hipGraph replay) fed by two DeviceLoaders against the same
    step on tensors resident before the step, alternated window by window in one process: ms per step each, and the
    spread between the windows of the resident-tensor step, which is the noise a difference has to exceed.
(c) The host path: a numpy restatement of the reference's per-sample recipe (normal_pc, x-rotation, z-rotation, float64
    jitter over all P points, shuffle of P indices, transpose) under torch.utils.data.DataLoader(num_workers=2, batch 32),
    in a process of its own that never opens the GPU (forked workers and a live HIP context do not mix)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, P = 4096, 2048
SHAPES = {'config2': {'N': 1024, 'batch': 32, 'dataset_type': 'scannet'}, 'config3': {'N': 2048, 'batch': 64, 'dataset_type': 'scannet'}}


def synth_dataset(m, p, seed):
    """Off-centre clouds in [-1, 1]^3 + offset, labels 0..9 (host arrays)."""
    g = np.random.RandomState(seed)
    pts = (g.uniform(-1, 1, size=(m, p, 3)) + g.uniform(-0.5, 0.5, size=(m, 1, 3))).astype(np.float32)
    return pts, g.randint(0, 10, size=m)


# ------------------------------------------------------------------------------------------------------ (c) host baseline
class HostRecipe(torch.utils.data.Dataset):
    """The reference's per-sample work, restated in numpy (fp32 normal_pc, float64 rotations and jitter)."""

    def __init__(self, pts, labels, num_points, pre_rotate=True, aug=True):
        self.pts, self.labels, self.n, self.pre_rotate, self.aug = pts, labels, num_points, pre_rotate, aug

    def __len__(self):
        return len(self.pts)

    def __getitem__(self, i):
        x = self.pts[i][:, :3]
        x = x - x.mean(axis=0)
        x = x / np.max(np.sqrt(np.sum(abs(x ** 2), axis=-1)))
        if self.pre_rotate:
            c, s = np.cos(-np.pi / 2), np.sin(-np.pi / 2)
            x = x.dot(np.asarray([[1, 0, 0], [0, c, -s], [0, s, c]])).astype('float32')
        if self.aug:
            a = np.random.uniform() * 2 * np.pi
            x = np.dot(x, np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]))
            x = np.clip(0.01 * np.random.randn(*x.shape), -0.05, 0.05) + x
        if x.shape[0] > self.n:
            order = np.arange(x.shape[0])
            np.random.shuffle(order)
            x = x[order[:self.n]]
        return torch.from_numpy(np.expand_dims(x.transpose(), axis=2)).type(torch.FloatTensor), self.labels[i]


def host_baseline(a):
    pts, labels = synth_dataset(M, P, 0)
    res = {}
    for name, s in SHAPES.items():
        loader = torch.utils.data.DataLoader(HostRecipe(pts, labels, s['N']), batch_size=32, shuffle=True, num_workers=2,
                                             drop_last=True)
        for _ in loader:                                     # one warm-up epoch: worker start-up, page faults
            pass
        t0 = time.perf_counter()
        n = 0
        for data, _ in loader:
            n += data.shape[0]
        dt = time.perf_counter() - t0
        res[name] = {'clouds_per_s': n / dt, 'us_per_batch_of_32': 1e6 * dt / (n / 32), 'clouds': n, 'num_workers': 2}
    print(json.dumps({'host_baseline': res}))


# ------------------------------------------------------------------------------------------------------ (a) loader alone
def loader_alone(a, dev):
    from sug_amd import ops
    from sug_amd.data.dataloader import DeviceLoader, UnifiedPointDG
    pts, labels = synth_dataset(M, P, 0)
    res = {}
    for name, s in SHAPES.items():
        ds = UnifiedPointDG(s['dataset_type'], pts, labels, pc_input_num=s['N'], aug=True, model='DGCNN', device=dev, seed=1)
        loader = DeviceLoader(ds, batch_size=s['batch'], shuffle=True, drop_last=True)
        for _ in loader:
            pass
        torch.cuda.synchronize()
        per_epoch = []
        for _ in range(a.epochs):
            t0 = time.perf_counter()
            for _ in loader:
                pass
            torch.cuda.synchronize()
            per_epoch.append(time.perf_counter() - t0)
        nb = len(loader)
        med = sorted(per_epoch)[len(per_epoch) // 2]
        # the kernel alone: back-to-back launches into one buffer
        B, N = s['batch'], s['N']
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        out = torch.empty(B, 3, N, device=dev)
        launch = lambda: ops.prepare_batch(ds.pts, idx, N, ds.pre_rotate, True, seed=1, counter=ds.counter, out=out)
        for _ in range(10):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            launch()
        e1.record()
        torch.cuda.synchronize()
        k_us = 1e3 * e0.elapsed_time(e1) / a.launches
        alg = 12 * B * (P + N)
        res[name] = {'P': P, 'N': N, 'batch': B, 'batches_per_epoch': nb, 'us_per_batch': 1e6 * med / nb,
                     'clouds_per_s': nb * B / med, 'epoch_s': per_epoch, 'kernel_us_back_to_back': k_us,
                     'algorithmic_bytes': alg, 'kernel_GBps': alg / k_us / 1e3}
    return res


# ------------------------------------------------------------------------------------------------------ (b) in front of the step
def step_fed(a, dev):
    from bench import BENCH_METHODS, synth
    from sug_amd.data.dataloader import DeviceLoader, UnifiedPointDG
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    B, N = 32, 1024
    torch.manual_seed(666)
    model = Net_MDA('DGCNN').to(dev).train()
    tr = SUGStep(model, lr=1e-3, weight_decay=5e-5, use_graph=True, methods=BENCH_METHODS)
    resident = synth(B, N, 666, dev)
    loaders = []
    for seed, kind in ((1, 'modelnet'), (2, 'scannet')):
        pts, labels = synth_dataset(M, P, seed)
        ds = UnifiedPointDG(kind, pts, labels, pc_input_num=N, aug=True, model='DGCNN', device=dev, seed=seed)
        loaders.append(DeviceLoader(ds, batch_size=B, shuffle=True, drop_last=True))
    its = [iter(l) for l in loaders]

    def fed():
        batch = []
        for i in (0, 1):
            try:
                d = next(its[i])
            except StopIteration:
                its[i] = iter(loaders[i])
                d = next(its[i])
            batch.extend(d)
        return tr.step(*batch)

    run = {'resident': lambda: tr.step(*resident), 'loader': fed}
    torch.manual_seed(666)
    for f in run.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    windows = {k: [] for k in run}
    for _ in range(a.windows):
        for k, f in run.items():                              # alternated: both see the same machine state
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            windows[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
    med = {k: sorted(w)[len(w) // 2] for k, w in windows.items()}
    return {'model': 'DGCNN', 'batch_per_domain': B, 'N': N, 'steps_per_window': a.steps, 'ms_per_step': med, 'windows_ms': windows,
            'resident_spread_ms': max(windows['resident']) - min(windows['resident']),
            'loader_minus_resident_ms': med['loader'] - med['resident']}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--launches', type=int, default=500)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--host-baseline', action='store_true')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'data_pipeline_bench.json'))
    a = ap.parse_args()
    if a.host_baseline:
        host_baseline(a)
        sys.exit(0)
    result = {}
    if not a.skip_host:              # first, in a child: this process has not touched the GPU yet
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--host-baseline'], capture_output=True, text=True,
                               timeout=900, env=dict(os.environ, HIP_VISIBLE_DEVICES='', OMP_NUM_THREADS='1'))
        if child.returncode != 0:
            raise RuntimeError('host baseline failed:\n' + child.stderr[-2000:])
        result.update(json.loads(child.stdout.strip().splitlines()[-1]))
    if not torch.cuda.is_available():
        raise RuntimeError('bench_data_pipeline needs a HIP device; there is no CPU path for (a) and (b)')
    dev = torch.device('cuda:0')
    result['device'] = torch.cuda.get_device_name(0)
    result['loader_alone'] = loader_alone(a, dev)
    result['step_fed'] = step_fed(a, dev)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
