#!/usr/bin/env python3
"""Generate tests/golden/cl_loss.npz by RUNNING THE REFERENCE (build container only, CPU, a few seconds).

Usage (from the repo root):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cl_goldens.py

The reference's model/mmd.py is imported with the stub modules of make_mmd_estimator_goldens.py, and its
contrastive_loss_weighted is called with the criterion its trainer builds, nn.CosineEmbeddingLoss(margin, reduction='none').
That function sends its one-hot labels and the weights .to(device='cuda'); for the duration of each call this process
answers such a request with the tensor where it is (no_cuda_request below) -- the one-hot labels take no part in the value.

Per shape (m, D) the file holds one pair of feature blocks, drawn on the fp16 grid and stored as fp16, the source labels,
and for each of the nine variants (label pattern, margin, weights) the target labels, the weights, the reference's fp32
value, its fp64 value (the same function on .double() inputs), val_err = |fp32 - fp64|, and for the gradient of both blocks
grad_err = max |grad32 - grad64| and grad_scale = max |grad64|.  The fp64 GRADIENTS are not stored: the tests recompute
them with the composed lines of sug_amd.model.mmd on the CPU in fp64, and this script asserts that those lines give the
reference's fp64 values and gradients on every case.

Condition on the inputs (asserted in fp64, the draw repeated otherwise): every row of every shape has |cos - margin| >= 1e-3
for every margin in use, so the clamp's kink is out of reach of fp32 rounding and the active rows are the same in fp32 and
fp64.  Row i of the target block is rho_i x_i + sqrt(1 - rho_i^2) noise with rho_i spread over [-0.3, 0.95]: negative pairs on
both sides of every margin.

Two degenerate cases stand alone (m = 2, D = 8, positive pairs, margin 0.2, no weights): 'zero' has a zero source row
(cos = 0, a gradient of order 1e6 times the other row's, finite); 'same' has x_i == y_i in both rows (a loss of order 1e-13).
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

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

# every m of (1, 2, 3, 33, 65) with every D of (1, 3, 70, 257, 4099) that the 200 KB of the file allow: the long rows with
# m = 1 and 3 (rows do not see each other), D = 257 up to m = 33
SHAPES = [(m, D) for m in (1, 2, 3, 33, 65) for D in (1, 3, 70)] + [(1, 257), (2, 257), (3, 257), (33, 257), (1, 4099), (3, 4099)]
MARGINS = (0.2, 0.0, 0.5)
LABELS = ('positive', 'negative', 'mixed')
WEIGHTS = ('none', 'positive', 'signed')
# (label pattern, margin, weights): every pair of two of the three settings occurs
VARIANTS = [(li, mi, (li + mi) % 3) for li in range(3) for mi in range(3)]
LABEL_WEIGHT = 0.3                        # takes no part in the value (model/mmd.py:83-88)


@contextlib.contextmanager
def no_cuda_request():
    real = torch.Tensor.to

    def to(self, *a, **k):
        if k.get('device', None) == 'cuda':
            k = {key: v for key, v in k.items() if key != 'device'}
        return real(self, *a, **k) if (a or k) else self

    torch.Tensor.to = to
    try:
        yield
    finally:
        torch.Tensor.to = real


def fp16_grid(t):
    return t.half().float()


def reference(ls, X, lt, Y, margin, w):
    crit = nn.CosineEmbeddingLoss(margin=margin, reduction='none')
    with no_cuda_request():
        return r_mmd.contrastive_loss_weighted(ls, X, lt, Y, LABEL_WEIGHT, crit, sample_weights=w)


def mirror(ls, X, lt, Y, margin, w):
    return mmd.contrastive_loss_weighted(ls, X, lt, Y, LABEL_WEIGHT, nn.CosineEmbeddingLoss(margin=margin, reduction='none'),
                                         sample_weights=w)


def value_and_grads(fn, ls, X, lt, Y, margin, w):
    X, Y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    v = fn(ls, X, lt, Y, margin, w)
    gx, gy = torch.autograd.grad(v, (X, Y), allow_unused=True)
    return v.detach(), torch.cat([torch.zeros_like(X) if g is None else g for g in (gx, gy)], 0)


def close64(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err, scale = float((a - b).abs().max()), max(float(b.abs().max()), 1e-300)
    assert err <= 1e-11 * scale, '%s: the mirror\'s composed lines differ from the reference in fp64 by %g (scale %g)' % (what, err, scale)


def cosines(X, Y):
    X, Y = X.double(), Y.double()
    return (X * Y).sum(1) / torch.sqrt(((X * X).sum(1) + 1e-12) * ((Y * Y).sum(1) + 1e-12))


def draw(m, D, g):
    while True:
        X = fp16_grid(torch.randn(m, D, generator=g) * 0.7)
        rho = torch.linspace(-0.3, 0.95, m)[torch.randperm(m, generator=g)] if m > 1 else torch.tensor([0.6])
        rho = (rho + 0.04 * torch.randn(m, generator=g)).clamp(-0.99, 0.99).unsqueeze(1)
        Y = fp16_grid(rho * X + torch.sqrt(1 - rho * rho) * torch.randn(m, D, generator=g) * 0.7)
        c = cosines(X, Y)
        if all(float((c - mg).abs().min()) >= 1e-3 for mg in MARGINS):
            return X, Y


def target_labels(ls, kind):
    other = (ls + 1 + torch.arange(ls.numel()) % 3) % 10
    assert not bool((other == ls).any())
    if kind == 'positive':
        return ls.clone()
    if kind == 'negative':
        return other
    return torch.where(torch.arange(ls.numel()) % 2 == 0, ls, other)


def weights(m, kind, g):
    if kind == 'none':
        return None
    w = fp16_grid(0.5 + torch.rand(1, m, generator=g))
    if kind == 'signed':
        w[0, 0] = 0.0
        w[0, m - 1] = -0.75
    return w


def record(out, key, ls, X, lt, Y, margin, w):
    """One case: run the reference in fp32 and fp64, pin the mirror's composed lines to it, return the stored numbers."""
    w64 = None if w is None else w.double()
    assert all(float(abs(c - margin)) >= 1e-3 for c, a, b in zip(cosines(X, Y), ls, lt) if int(a) != int(b)), key
    v32, g32 = value_and_grads(reference, ls, X, lt, Y, margin, w)
    v64, g64 = value_and_grads(reference, ls, X.double(), lt, Y.double(), margin, w64)
    assert v32.dtype == torch.float32 and v64.dtype == torch.float64 and bool(torch.isfinite(g64).all()), key
    mv, mg = value_and_grads(mirror, ls, X.double(), lt, Y.double(), margin, w64)
    close64(mv, v64, key + ' value')
    close64(mg, g64, key + ' gradient')
    mv32, _ = value_and_grads(mirror, ls, X, lt, Y, margin, w)
    assert abs(float(mv32) - float(v32)) <= 1e-6 * max(1.0, abs(float(v32))), key
    return (float(v32), float(v64), abs(float(v32) - float(v64)), float((g32.double() - g64).abs().max()), float(g64.abs().max()))


def main():
    g = torch.Generator().manual_seed(20261)
    out = {'shapes': np.asarray(SHAPES, dtype=np.int64), 'margins': np.asarray(MARGINS, dtype=np.float64),
           'variants': np.asarray(VARIANTS, dtype=np.int64), 'label_kinds': np.asarray(LABELS), 'weight_kinds': np.asarray(WEIGHTS)}
    for si, (m, D) in enumerate(SHAPES):
        X, Y = draw(m, D, g)
        ls = torch.randint(0, 10, (m,), generator=g)
        wsets = [weights(m, kind, g) for kind in WEIGHTS]
        key = 's%d_' % si
        out[key + 'X'], out[key + 'Y'], out[key + 'ls'] = X.half(), Y.half(), ls
        out[key + 'lt'] = torch.stack([target_labels(ls, kind) for kind in LABELS])
        out[key + 'w'] = torch.cat(wsets[1:], 0)                                  # [2, m]: 'positive', 'signed'
        rows = []
        for vi, (li, mi, wi) in enumerate(VARIANTS):
            rows.append(record(out, '%s%d' % (key, vi), ls, X, out[key + 'lt'][li], Y, MARGINS[mi], wsets[wi]))
        rows = np.asarray(rows, dtype=np.float64)
        out[key + 'v32'] = rows[:, 0].astype(np.float32)
        out[key + 'v64'], out[key + 'val_err'], out[key + 'grad_err'], out[key + 'grad_scale'] = rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4]
        print('m=%-3d D=%-5d  values %s  rel grad err %.1e' % (m, D, ' '.join('%.4f' % v for v in rows[:, 1]),
                                                              float((rows[:, 3] / np.maximum(rows[:, 4], 1e-300)).max())))
    # the two degenerate cases
    Xz = fp16_grid(torch.randn(2, 8, generator=g) * 0.7)
    Yz = fp16_grid(torch.randn(2, 8, generator=g) * 0.7)
    Xz[0] = 0.0
    Xs = fp16_grid(torch.randn(2, 8, generator=g) * 0.7)
    lab = torch.tensor([3, 7])
    for name, X, Y in (('zero', Xz, Yz), ('same', Xs, Xs.clone())):
        r = record(out, name, lab, X, lab, Y, 0.2, None)
        key = 'd_%s_' % name
        out[key + 'X'], out[key + 'Y'], out[key + 'ls'] = X.half(), Y.half(), lab
        out[key + 'v32'] = np.asarray(r[0], dtype=np.float32)
        out[key + 'v64'], out[key + 'val_err'], out[key + 'grad_err'], out[key + 'grad_scale'] = (np.asarray(v) for v in r[1:])
        print('degenerate %-4s  fp32 %.6g  fp64 %.6g  grad scale %.3g  grad err %.3g' % (name, r[0], r[1], r[4], r[3]))
    _, gz = value_and_grads(reference, lab, Xz.double(), lab, Yz.double(), 0.2, None)
    assert float(gz[0].abs().max()) > 1e5 * float(gz[1].abs().max()), 'the zero row should dominate the gradient'
    assert 0.0 < float(out['d_same_v64']) < 1e-11
    conv = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'cl_loss.npz')
    np.savez_compressed(path, **conv)
    print('wrote %s  %.1f KB' % (path, os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == '__main__':
    main()
