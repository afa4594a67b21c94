#!/usr/bin/env python3
"""What the KPConv capacity layout (KPConv_g.set_level_caps) buys a SUG training step on one GPU.
Prints one JSON line and writes it to --out.

Workload: Net_MDA('KPConv'), 16 clouds per domain, N = 1024, the benchmark's synthetic normalised clouds (8 batches, fed in
turn, so the level sizes change from step to step), bench.BENCH_METHODS.  Caps: calibrate_level_caps over the 8 batches.
Legs, in ONE process, alternated `--rounds` times (each leg trains a model of its own from the same initial weights):
  caller  the caller's loop as it runs without caps: four eager model(...) calls on the exact-size path (one host wait each),
          the composed losses, loss.backward() and three torch.optim.Adam updates (train_dg_single_gpu.py:191-203, :260-335)
  eager   SUGStep with caps, use_graph=False
  replay  SUGStep with caps, use_graph=True (planned, captured and replayed before any clock starts)
Per leg: ms per step from device events around every step (`--steps` steps per round after `--warmup`): the median over all
rounds, the quartiles, the medians of the rounds and their spread (max - min) / median; host waits per step (warnings of
torch.cuda.set_sync_debug_mode('warn') over 4 further steps); per level the valid rows over the capacity (mean and largest
over the 8 batches, for the paired batch of 32 clouds the SUGStep legs run).
Kernel dispatches per step (--launches; runs of their own in child processes, added to the record in --out): the dispatches
of `rocprofv3 --kernel-trace --stats` runs of 2 and 6 steps after the warm-up, the difference over 4, with the kernel time
per step and the eight kernels that take most of it.  The replay leg hands the host ONE graph launch per step, whatever the
number of kernel nodes in it.

Usage: python tools/bench_kpconv_caps.py [--rounds 3] [--steps 50] [--warmup 5] [--launches]
                                         [--out profiles/kpconv_caps_bench.json]"""
import argparse
import csv
import gc
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B, N, BATCHES = 16, 1024, 8
LEGS = ('caller', 'eager', 'replay')


def _batches():
    import torch
    from oracle import ref_cpu as O
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(BATCHES):
        data, data_t = O.synth_clouds(B, N, g).cuda(), O.synth_clouds(B, N, g).cuda()
        lab, lab_t = torch.randint(0, 10, (B,), generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()
        out.append((data, lab, data_t, lab_t))
    return out


def _caller_step(model, methods):
    """The four-call loop of an unchanged caller (train_dg_single_gpu.py:260-335) on the exact-size path."""
    import torch
    from sug_amd.model import mmd
    M = methods
    crit = torch.nn.CrossEntropyLoss()
    lr, wd = 1e-3, 5e-5
    opt_g = torch.optim.Adam([{'params': v} for k, v in model.g.named_parameters() if 'pred_offset' not in k], lr=lr, weight_decay=wd)
    opt_c = torch.optim.Adam([{'params': model.c1.parameters()}, {'params': model.c2.parameters()}], lr=lr, weight_decay=wd)
    opt_dis = torch.optim.Adam([{'params': model.g.parameters()}, {'params': model.attention_s.parameters()},
                                {'params': model.attention_t.parameters()}], lr=lr, weight_decay=wd)
    geo, sem = M['GEO_MMD'][0], M['SEM_MMD'][0]

    def step(data, label, data_t, label_t):
        ps1, ps2, fs1, fs2 = model(data, semantic_adaption=True)
        pt1, pt2, ft1, ft2 = model(data_t, semantic_adaption=True)
        loss = M['CLS_WEIGHT'] * M['SRC_LOSS_WEIGHT'] * 0.5 * (crit(ps1, label) + crit(ps2, label))
        node_s = model(data, node_adaptation_s=True)
        node_t = model(data_t, node_adaptation_t=True)
        loss = loss + M['MMD_WEIGHT'] * geo['GEO_SCALE'] * mmd.mmd_cal(label, node_s, label_t, node_t, geo, data_s=data, data_t=data_t)
        loss = loss + 0.5 * M['MMD_WEIGHT'] * sem['SEM_SCALE'] * (
            mmd.mmd_cal(label, fs1, label_t, ft1, sem, data_s=ps1, data_t=pt1) +
            mmd.mmd_cal(label, fs2, label_t, ft2, sem, data_s=ps2, data_t=pt2))
        loss.backward()
        opt_dis.step()
        opt_g.step()
        opt_c.step()
        opt_g.zero_grad()
        opt_c.zero_grad()
        opt_dis.zero_grad()
        return loss.detach()
    return step


def _legs(caps, only=None):
    """{leg: step(batch)} -- every leg on a model of its own, from the same initial weights."""
    import torch
    import bench
    from oracle import ref_cpu as O
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep, METHODS
    methods = dict(METHODS)
    methods.update(bench.BENCH_METHODS)
    torch.manual_seed(0)
    ref = Net_MDA('KPConv')
    sd = O.fill_params({k: tuple(v.shape) for k, v in ref.state_dict().items() if 'kernel_points' not in k}, 5)
    sd.update({k: v for k, v in ref.state_dict().items() if 'kernel_points' in k})
    legs, models = {}, {}
    for leg in LEGS:
        if only is not None and leg != only:
            continue
        m = Net_MDA('KPConv')
        m.load_state_dict(sd)
        m = m.cuda().train()
        models[leg] = m
        if leg == 'caller':
            fn = _caller_step(m, methods)
            legs[leg] = lambda batch, fn=fn: fn(*batch)
        else:
            m.g.set_level_caps(caps)
            tr = SUGStep(m, lr=1e-3, weight_decay=5e-5, use_graph=(leg == 'replay'), methods=bench.BENCH_METHODS)
            legs[leg] = lambda batch, tr=tr: tr.step(*batch)
    return legs, models


def _calibrate(batches):
    """(caps over the 8 batches, per level [total rows of the paired 32-cloud batch] per batch)."""
    import torch
    from sug_amd.model.KPConv_model import calibrate_level_caps, PreprocessorGPU, KPConvConfig, _split_clouds
    caps = calibrate_level_caps([t for b in batches for t in (b[0], b[2])])
    pre = PreprocessorGPU(KPConvConfig)
    totals = []
    for b in batches:
        meta = pre.forward_packed(*_split_clouds(torch.cat((b[0], b[2]))))
        totals.append([sum(l) for l in meta['lengths']])
    return caps, totals


def _time_round(step, batches, steps, warmup, start):
    import torch
    for i in range(warmup):
        step(batches[(start + i) % BATCHES])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    gc.collect()
    gc.disable()
    try:
        for i, (a, b) in enumerate(ev):
            a.record()
            step(batches[(start + warmup + i) % BATCHES])
            b.record()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return [a.elapsed_time(b) for a, b in ev]


def _host_waits(step, batches):
    import torch
    try:
        torch.cuda.set_sync_debug_mode('warn')
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            for i in range(4):
                step(batches[i])
        return sum('synchroniz' in str(w.message).lower() for w in seen) / 4.0
    finally:
        torch.cuda.set_sync_debug_mode('default')
        torch.cuda.synchronize()


def child_steps(leg, steps, warmup):
    """`steps` steps of one leg after the warm-up (run under rocprofv3 by the parent process)."""
    import torch
    batches = _batches()
    caps, _ = _calibrate(batches)
    legs, _ = _legs(caps, only=leg)
    for i in range(warmup + steps):
        legs[leg](batches[i % BATCHES])
    torch.cuda.synchronize()
    return {}


def _launches(leg, steps, warmup, limit):
    """Kernel dispatches of a run of warmup + `steps` steps of one leg (rocprofv3 --kernel-trace --stats)."""
    tmp = tempfile.mkdtemp(prefix='kpconv_caps_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--child', '--leg', leg, '--steps', str(steps), '--warmup', str(warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
        if r.returncode != 0:
            raise RuntimeError('rocprofv3 run ended with %d:\n%s' % (r.returncode, r.stderr.decode()[-3000:]))
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if len(files) != 1:
            raise RuntimeError('expected one kernel_stats.csv, found %s' % files)
        rows = list(csv.DictReader(open(files[0])))
        key = lambda row, *names: next(row[c] for c in row if c.strip().lower() in names)
        per = {}
        for row in rows:
            c, ns = per.get(key(row, 'name', 'kernel'), (0, 0))
            per[key(row, 'name', 'kernel')] = (c + int(key(row, 'calls', 'count')), ns + int(float(key(row, 'totaldurationns', 'total_duration_ns', 'total'))))
        return per
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'kpconv_caps_bench.json'))
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--leg')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_steps(a.leg, a.steps, a.warmup)))
        return
    res = {'workload': "SUG step, Net_MDA('KPConv'), %d clouds per domain, N = %d, %d synthetic batches in turn, BENCH_METHODS"
                       % (B, N, BATCHES), 'dtype': 'fp32',
           'legs': {'caller': 'four eager model(...) calls on the exact-size path, loss.backward(), three torch.optim.Adam updates',
                    'eager': 'SUGStep with level caps, use_graph=False', 'replay': 'SUGStep with level caps, use_graph=True'},
           'rounds': a.rounds, 'steps_per_round': a.steps, 'warmup_per_round': a.warmup}
    failed = None
    try:
        if a.launches:                                      # child processes only: this process does not touch the GPU
            if a.out and os.path.exists(a.out):             # added to the timing run's record
                with open(a.out) as fh:
                    res = json.loads(fh.read())
            res['kernel_dispatches_per_step'], res['kernel_ms_per_step'], res['top_kernels'] = {}, {}, {}
            for leg in LEGS:
                lo, hi = (_launches(leg, s, a.warmup, 600) for s in (2, 6))
                d = {k: ((hi[k][0] - lo.get(k, (0, 0))[0]) / 4.0, (hi[k][1] - lo.get(k, (0, 0))[1]) / 4e6) for k in hi}
                res['kernel_dispatches_per_step'][leg] = round(sum(v[0] for v in d.values()), 2)
                res['kernel_ms_per_step'][leg] = round(sum(v[1] for v in d.values()), 3)
                top = sorted(d.items(), key=lambda kv: -kv[1][1])[:8]
                res['top_kernels'][leg] = [{'kernel': k[:60], 'calls_per_step': round(v[0], 2), 'ms_per_step': round(v[1], 3)}
                                           for k, v in top]
        else:
            import torch
            from sug_amd.model.KPConv_model import level_capacity
            batches = _batches()
            caps, totals = _calibrate(batches)
            C = level_capacity(2 * B, N, caps)
            res['level_caps'] = list(caps)
            res['levels'] = [{'level': l, 'capacity': C[l], 'valid_over_capacity_mean': round(statistics.mean(t[l] for t in totals) / C[l], 4),
                              'valid_over_capacity_max': round(max(t[l] for t in totals) / C[l], 4)} for l in range(1, len(C))]
            legs, models = _legs(caps)
            ms = {leg: [] for leg in LEGS}
            for r in range(a.rounds):
                for leg in LEGS:                            # the legs alternate within a round
                    ms[leg].append(_time_round(legs[leg], batches, a.steps, a.warmup, r * (a.steps + a.warmup)))
            res['results'] = {}
            for leg in LEGS:
                flat = sorted(v for w in ms[leg] for v in w)
                med = statistics.median(flat)
                per_round = [statistics.median(w) for w in ms[leg]]
                q = statistics.quantiles(flat, n=4)
                res['results'][leg] = {'ms_per_step_median': round(med, 3), 'ms_per_step_q1_q3': [round(q[0], 3), round(q[2], 3)],
                                       'ms_per_step_min_max': [round(flat[0], 3), round(flat[-1], 3)],
                                       'round_medians_ms': [round(v, 3) for v in per_round],
                                       'spread_between_rounds': round((max(per_round) - min(per_round)) / med, 4),
                                       'host_waits_per_step': _host_waits(legs[leg], batches)}
            for leg in ('eager', 'replay'):
                rep = models[leg].g.capacity_report()
                res['results'][leg]['overflows'] = rep['overflows']
                res['results'][leg]['rows_needed_max'] = [l['needed'] for l in rep['levels']]
            a_, c_ = res['results']['caller'], res['results']['replay']
            res['replay_below_caller_ms'] = round(a_['ms_per_step_median'] - c_['ms_per_step_median'], 3)
            res['caller_spread_ms'] = round(a_['spread_between_rounds'] * a_['ms_per_step_median'], 3)
            torch.cuda.synchronize()
    except (RuntimeError, StopIteration, subprocess.TimeoutExpired) as e:
        failed = res['error'] = str(e)[-1500:]
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)
    if failed is not None:
        sys.exit(1)


if __name__ == '__main__':
    main()
