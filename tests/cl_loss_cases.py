"""Shared by tests/test_cl_loss_host.py and tests/test_gpu_cl_loss.py: the cases of tests/golden/cl_loss.npz and their fp64
references, computed once, on the CPU, with the composed lines of sug_amd.model.mmd -- which make_cl_goldens.py proved
equal to the reference's contrastive_loss_weighted in fp64, and whose fp64 values the fixture pins."""
import functools

import torch
import torch.nn as nn

from conftest import load_golden

DEGENERATE = ('zero', 'same')


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden('cl_loss.npz')


def shapes():
    return [(int(m), int(D)) for m, D in golden()['shapes'].tolist()]


def shape_ids():
    return ['m%d-D%d' % s for s in shapes()]


def variants():
    """[(label pattern index, margin, weight set index)] -- weight set 0 is 'no weights'."""
    G = golden()
    return [(int(li), float(G['margins'][int(mi)]), int(wi)) for li, mi, wi in G['variants'].tolist()]


def case(si, vi):
    """(label_s, X, label_t, Y, margin, weights or None) of variant vi of shape si: fp32 features, fp32 weights [1, m]."""
    G = golden()
    li, margin, wi = variants()[vi]
    key = 's%d_' % si
    w = None if wi == 0 else G[key + 'w'][wi - 1:wi].float()
    return G[key + 'ls'], G[key + 'X'].float(), G[key + 'lt'][li], G[key + 'Y'].float(), margin, w


def recorded(si, vi):
    """(v32, v64, val_err, grad_err, grad_scale) of the reference."""
    G = golden()
    key = 's%d_' % si
    return tuple(float(G[key + f][vi]) for f in ('v32', 'v64', 'val_err', 'grad_err', 'grad_scale'))


def degenerate(name):
    G = golden()
    key = 'd_%s_' % name
    return G[key + 'ls'], G[key + 'X'].float(), G[key + 'ls'], G[key + 'Y'].float(), 0.2, None


def degenerate_recorded(name):
    G = golden()
    key = 'd_%s_' % name
    return tuple(float(G[key + f]) for f in ('v32', 'v64', 'val_err', 'grad_err', 'grad_scale'))


def criterion(margin):
    return nn.CosineEmbeddingLoss(margin=margin, reduction='none')


def composed(ls, X, lt, Y, margin, w, dtype=torch.float64):
    """(value, [d X ; d Y]) of the mirror's composed lines on CPU tensors of `dtype`."""
    from sug_amd.model import mmd
    X, Y = X.to(dtype).requires_grad_(True), Y.to(dtype).requires_grad_(True)
    v = mmd.contrastive_loss_weighted(ls, X, lt, Y, 0.3, criterion(margin), sample_weights=None if w is None else w.to(dtype))
    gx, gy = torch.autograd.grad(v, (X, Y), allow_unused=True)
    return v.detach(), torch.cat([torch.zeros_like(X) if g is None else g for g in (gx, gy)], 0)


@functools.lru_cache(maxsize=None)
def ref64(si, vi):
    return composed(*case(si, vi))


@functools.lru_cache(maxsize=None)
def degenerate_ref64(name):
    return composed(*degenerate(name))
