#!/usr/bin/env python3
"""Generate tests/golden/mmd_estimators.npz by RUNNING THE REFERENCE (build container only, CPU, a few seconds).

Usage (from the repo root):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mmd_estimator_goldens.py

The reference's model/mmd.py is imported with the stub modules of make_goldens.py.  For every case the file holds the
inputs, the reference's fp32 outputs, its fp64 outputs (the same functions on .double() inputs) and
ref_err = |fp32 - fp64| per quantity -- for the gradients as two scalars per upstream, max |grad32 - grad64| and
max |grad64|.  The inputs are drawn on the fp16 grid and stored as fp16 (random fp32 blocks do not compress).  The fp64
GRADIENTS are not stored (every case, three upstreams, both estimators: 2.6 MB): the tests recompute them with the composed
lines of sug_amd.model.mmd on the CPU in fp64, and this script asserts that those lines give the reference's fp64 values
and gradients on every case, so the stored fp64 values pin them at test time.

Ratio cases: X = randn s, Y = randn s + shift; no case's fp64 var_est sits at the clamp (asserted: <= 0 or >= 1e-6).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('SUG_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

for name in ('tkinter', 'turtle', 'chamfer_distance', 'h5py', 'easydict', 'tensorboardX'):
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)
sys.modules['turtle'].distance = None
sys.modules['chamfer_distance'].ChamferDistance = None
sys.modules['easydict'].EasyDict = dict
sys.modules['tensorboardX'].SummaryWriter = object

import model.mmd as r_mmd                 # noqa: E402  (reference)
from sug_amd.model import mmd             # noqa: E402  (the mirror: CPU tensors take its composed lines)

torch.set_num_threads(8)

RATIO_CASES = [(2, 3, 1, .5), (3, 5, 1, .5), (5, 7, .5, .3), (8, 16, .3, .2), (8, 16, 3, 1), (33, 70, .2, .1),
               (64, 257, .1, .05), (65, 129, .05, .02)]
ADJ_SHAPES = [(m, D) for m in (2, 3, 33) for D in (1, 70)]
# (d, alpha, c); d = 0 marks linear_mmd2.  (2, 0.5, -3) and (3, -0.7, 0.25): negative bases; d = 2.5: the composed path
ADJ_PARAMS = [(0, 0, 0), (1, 1.0, 2.0), (2, 1.0, 2.0), (3, 1.0, 2.0), (2, 0.5, -3.0), (3, -0.7, 0.25), (2.5, 0.05, 2.0)]
UPSTREAMS = 3


def fp16_grid(t):
    return t.half().float()


def grads(fn, X, Y, k=None):
    X, Y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    out = fn(X, Y)
    out = out[k] if k is not None else out
    return torch.cat(torch.autograd.grad(out, (X, Y)), 0)


def close64(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err, scale = float((a - b).abs().max()), max(float(b.abs().max()), 1e-300)
    assert err <= 1e-11 * scale, '%s: the mirror\'s composed lines differ from the reference in fp64 by %g (scale %g)' % (what, err, scale)


def main():
    g = torch.Generator().manual_seed(20260)
    out = {'ratio_cases': np.asarray(RATIO_CASES, dtype=np.float64), 'adj_shapes': np.asarray(ADJ_SHAPES, dtype=np.int64),
           'adj_params': np.asarray(ADJ_PARAMS, dtype=np.float64)}
    sig = r_mmd.sigma_list
    for ci, (m, D, s, shift) in enumerate(RATIO_CASES):
        X = fp16_grid(torch.randn(m, D, generator=g) * s)
        Y = fp16_grid(torch.randn(m, D, generator=g) * s + shift)
        out['r%d_X' % ci], out['r%d_Y' % ci] = X.half(), Y.half()
        for b in (0, 1):
            ref = lambda A, B: r_mmd.mix_rbf_mmd2_and_ratio(A, B, sig, biased=bool(b))
            mir = lambda A, B: mmd.mix_rbf_mmd2_and_ratio(A, B, sig, biased=bool(b))
            o32 = torch.stack([v.double() for v in ref(X, Y)])
            o64 = torch.stack(list(ref(X.double(), Y.double())))
            close64(torch.stack(list(mir(X.double(), Y.double()))), o64, 'ratio case %d values' % ci)
            var = float(o64[2])
            assert var <= 0 or var >= 1e-6, 'case %d biased=%d: var_est %g sits at the clamp' % (ci, b, var)
            gerr, gscale = [], []
            for k in range(UPSTREAMS):
                g64 = grads(ref, X.double(), Y.double(), k)
                close64(grads(mir, X.double(), Y.double(), k), g64, 'ratio case %d gradient %d' % (ci, k))
                gerr.append(float((grads(ref, X, Y, k).double() - g64).abs().max()))
                gscale.append(float(g64.abs().max()))
            key = 'r%d_b%d_' % (ci, b)
            out[key + 'out32'], out[key + 'out64'] = o32.float(), o64
            out[key + 'val_err'] = (o32 - o64).abs()
            out[key + 'grad_err'], out[key + 'grad_scale'] = np.asarray(gerr), np.asarray(gscale)
            print('ratio m=%-3d D=%-4d biased=%d  mmd2 %.6g  var %.4g (%s)  rel err var %.1e  grad %s' % (
                m, D, b, float(o64[1]), var, 'clamped' if var < 1e-8 else 'open', float(out[key + 'val_err'][2]) / abs(var),
                ' '.join('%.1e' % (e / sc) for e, sc in zip(gerr, gscale))))
    for si, (m, D) in enumerate(ADJ_SHAPES):
        X = fp16_grid(torch.randn(m, D, generator=g) * 0.6)
        Y = fp16_grid(torch.randn(m, D, generator=g) * 0.6 + 0.3)
        out['a%d_X' % si], out['a%d_Y' % si] = X.half(), Y.half()
        for pi, (d, alpha, c) in enumerate(ADJ_PARAMS):
            d = int(d) if float(d).is_integer() else d
            if d == 0:
                ref, mir = r_mmd.linear_mmd2, mmd.linear_mmd2
            else:
                ref = lambda A, B: r_mmd.poly_mmd2(A, B, d=d, alpha=alpha, c=c)
                mir = lambda A, B: mmd.poly_mmd2(A, B, d=d, alpha=alpha, c=c)
            v32, v64 = ref(X, Y).double(), ref(X.double(), Y.double())
            assert bool(torch.isfinite(v64)), (si, pi)
            close64(mir(X.double(), Y.double()), v64, 'adjacent %d/%d value' % (si, pi))
            g64 = grads(ref, X.double(), Y.double())
            close64(grads(mir, X.double(), Y.double()), g64, 'adjacent %d/%d gradient' % (si, pi))
            key = 'a%d_p%d_' % (si, pi)
            out[key + 'v32'], out[key + 'v64'] = v32.float(), v64
            out[key + 'grad_err'] = np.asarray(float((grads(ref, X, Y).double() - g64).abs().max()))
            out[key + 'grad_scale'] = np.asarray(float(g64.abs().max()))
    # one row per domain: what the reference does there (the mirror sends it through its composed lines)
    X1, Y1 = torch.randn(1, 4, generator=g), torch.randn(1, 4, generator=g)
    for fn, name in ((r_mmd.linear_mmd2, 'linear'), (r_mmd.poly_mmd2, 'poly')):
        v = fn(X1, Y1)
        assert bool(torch.isnan(v)), name
    try:
        r_mmd.mix_rbf_mmd2_and_ratio(X1, Y1, sig)
        one_row = 'value'
    except ZeroDivisionError:
        one_row = 'ZeroDivisionError'
    out['ratio_one_row'] = np.asarray([one_row])
    print('m = 1: linear / poly NaN, ratio:', one_row)
    conv = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'mmd_estimators.npz')
    np.savez_compressed(path, **conv)
    print('wrote %s  %.1f KB' % (path, os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == '__main__':
    main()
