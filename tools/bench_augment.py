#!/usr/bin/env python3
"""What the scale / rotation-perturbation / shift stages of the data pipeline cost, and that the old stage set costs what it
did: the kernel alone at the config-2 shape (P 2048 -> N 1024, batch 32, pre-rotation on, in-kernel draws), device events
around back-to-back launches into one buffer, three variants alternated window by window in one process:

(a) sug_prepare_batch of the PARENT commit's library (--parent-lib: libsug_amd.so built from the commit this change sits
    on, e.g. `git worktree add ../parent HEAD~1 && make -C ../parent/sug_amd/csrc`), normalise + z-rotation + jitter;
(b) sug_prepare_batch of this tree's library, the same stages;
(c) sug_prepare_batch_aug of this tree's library with scale, perturbation and shift on as well.

    python tools/bench_augment.py --parent-lib ../parent/sug_amd/libsug_amd.so [--out profiles/augment_bench.json]

The gate: the new stages are uniform branches on kernel arguments, so the median of (b) may exceed the median of (a) by no
more than the spread (max - min) between (a)'s own windows; both are recorded, and the exit status is 1 when it fails.
(c) is reported, not gated.  Both libraries get the same arguments through ctypes, and (a) and (b) must write the same
bits."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, P, N, B = 256, 2048, 1024, 32


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True)
    ap.add_argument('--launches', type=int, default=20000, help='per window (about half a second)')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('bench_augment needs a HIP device; there is no CPU path')
    from sug_amd import _lib, ops
    new = _lib.lib()
    old = ctypes.CDLL(os.path.abspath(a.parent_lib))
    old.sug_prepare_batch.argtypes = _lib.DECLARATIONS['sug_prepare_batch'][1]
    old.sug_prepare_batch.restype = ctypes.c_int
    if hasattr(old, 'sug_prepare_batch_aug'):
        raise RuntimeError('%s already has sug_prepare_batch_aug: it is not the parent commit\'s library' % a.parent_lib)

    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    pts = (torch.rand(M, P, 3, generator=g) * 2 - 1 + (torch.rand(M, 1, 3, generator=g) - 0.5)).to(dev)
    idx = torch.randperm(M, generator=g)[:B].to(torch.int32).to(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = {k: torch.empty(B, 3, N, device=dev) for k in 'abc'}
    pre = (ctypes.c_float * 9)(*ops._PRE_ROTATE_X)
    params = (ctypes.c_float * ops.PREP_AUG_PARAMS)()
    for slot, v in zip(ops._PREP_AUG_SLOTS, (0.8, 1.25, 0.1, 0.06, 0.18)):
        params[slot] = v
    p, st = ops._p, ops._st
    old_stages = ops.PREP_NORMALIZE | ops.PREP_ROTATE_Z | ops.PREP_JITTER
    all_stages = old_stages | ops.PREP_SCALE | ops.PREP_PERTURB | ops.PREP_SHIFT

    def base(L, out):
        return lambda: L.sug_prepare_batch(p(pts), M, P, p(idx), B, N, old_stages, pre, None, None, None, 1, p(counter), 0.01, 0.05,
                                           p(out), None, None, None, st())

    run = {'a_parent_prepare_batch': base(old, outs['a']), 'b_prepare_batch': base(new, outs['b']),
           'c_prepare_batch_aug_all_stages': lambda: new.sug_prepare_batch_aug(
               p(pts), M, P, p(idx), B, N, all_stages, pre, None, None, None, None, None, None, 1, p(counter), 0.01, 0.05, params,
               p(outs['c']), None, None, None, None, None, None, st())}
    for k, f in run.items():
        for _ in range(200):
            if f() != 0:
                raise RuntimeError('%s failed: %s' % (k, (old if k[0] == 'a' else new).sug_last_error()))
    torch.cuda.synchronize()
    same = torch.equal(outs['a'], outs['b'])
    windows = {k: [] for k in run}
    for _ in range(a.windows):
        for k, f in run.items():                              # alternated: every variant sees the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            windows[k].append(1e3 * e0.elapsed_time(e1) / a.launches)
    med = {k: sorted(w)[len(w) // 2] for k, w in windows.items()}
    wa = windows['a_parent_prepare_batch']
    spread = max(wa) - min(wa)
    excess = med['b_prepare_batch'] - med['a_parent_prepare_batch']
    result = {'device': torch.cuda.get_device_name(0), 'shape': {'M': M, 'P': P, 'N': N, 'batch': B, 'pre_rotation': True},
              'launches_per_window': a.launches, 'kernel_us_back_to_back': med, 'windows_us': windows,
              'a_window_spread_us': spread, 'b_minus_a_us': excess, 'gate_b_minus_a_within_a_spread': bool(excess <= spread),
              'a_equals_b_bitwise': bool(same),
              'c_minus_b_us': med['c_prepare_batch_aug_all_stages'] - med['b_prepare_batch']}
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    sys.exit(0 if result['gate_b_minus_a_within_a_spread'] and same else 1)
