#!/usr/bin/env python3
"""Net_MDA('KPConv') forward + backward at 16 clouds of 1024 points: the build (HIP kernels) against a plain-torch
restatement of the same packed computation (same preprocessing metadata, same weights) on the same GPU.  Prints one
JSON line.  Usage: python tools/bench_kpconv.py [--steps 20] [--warmup 5] [--only-build]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_forward(m, x):
    """Plain torch on the build's metadata: gather-based KPConv (the reference's formulation), per-cloud instance norm
    by loops over the clouds, max pool by gather, global average by loops."""
    from sug_amd.model.KPConv_blocks import UnaryBlock
    from sug_amd.model.KPConv_model import _split_clouds
    import torch.nn.functional as F
    g = m.g
    pts, lengths = _split_clouds(x)
    meta = g.preprocessor.forward_packed(pts, lengths)
    L = meta['lengths']

    def inorm(v, lens):
        return torch.cat([F.instance_norm(s.t().unsqueeze(0)).squeeze(0).t() for s in torch.split(v, lens)])

    def kpconv(conv, q, s, nbr, v):
        nbr = nbr.long()
        sp = torch.cat((s, torch.full_like(s[:1], 1e6)))
        nb = sp[nbr] - q.unsqueeze(1)
        w = torch.clamp(1 - (nb.unsqueeze(2) - conv.kernel_points).pow(2).sum(3).sqrt() / conv.KP_extent, min=0)
        vx = torch.cat((v, torch.zeros_like(v[:1])))[nbr]
        wf = torch.matmul(w.transpose(1, 2), vx)
        out = (wf.permute(1, 0, 2) @ conv.weights).sum(0)
        cnt = torch.clamp((vx.sum(-1) > 0).sum(-1), min=1)
        return out / cnt.unsqueeze(1)

    def unary(u, v, lens, relu):
        y = inorm(v @ u.mlp.weight.t(), lens)
        return F.leaky_relu(y, 0.1) if relu else y

    v = meta['points'][0][:, 0:1]
    mid = None
    for i, blk in enumerate(g.encoder.encoder_blocks):
        l = blk.layer_ind
        strided = 'strided' in blk.block_name
        q = meta['points'][l + 1] if strided else meta['points'][l]
        nbr = meta['pools'][l] if strided else meta['neighbors'][l]
        lens = L[l + 1] if strided else L[l]
        if blk.__class__.__name__ == 'SimpleBlock':
            v = F.leaky_relu(inorm(kpconv(blk.KPConv, q, meta['points'][l], nbr, v), lens), 0.1)
        else:
            h = unary(blk.unary1, v, L[l], True) if isinstance(blk.unary1, UnaryBlock) else v
            h = F.leaky_relu(inorm(kpconv(blk.KPConv, q, meta['points'][l], nbr, h), lens), 0.1)
            h = unary(blk.unary2, h, lens, False)
            sc = torch.cat((v, torch.zeros_like(v[:1])))[nbr.long()].max(1)[0] if strided else v
            if isinstance(blk.unary_shortcut, UnaryBlock):
                sc = unary(blk.unary_shortcut, sc, lens, False)
            v = F.leaky_relu(h + sc, 0.1)
        if i == 2:
            mid = v
    feat = torch.stack([s.mean(0) for s in torch.split(v, L[-1])])
    return m.c1(feat), m.c2(feat), mid


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--clouds', type=int, default=16)
    ap.add_argument('--only-build', action='store_true')
    a = ap.parse_args()
    from oracle import ref_cpu as O
    from sug_amd.model.Model import Net_MDA
    torch.manual_seed(0)
    m = Net_MDA('KPConv').cuda().train()
    x = O.synth_clouds(a.clouds, 1024, torch.Generator().manual_seed(0)).cuda()

    def build_step():
        y1, y2 = m(x)
        (y1.sum() + y2.sum()).backward()

    def torch_step():
        y1, y2, _ = torch_forward(m, x)
        (y1.sum() + y2.sum()).backward()

    res = {'workload': 'Net_MDA(KPConv) fwd+bwd', 'clouds': a.clouds, 'N': 1024}
    res['build_ms'] = round(timed(build_step, a.steps, a.warmup), 3)
    if not a.only_build:
        with torch.no_grad():
            yb = m(x)[0]
            yt = torch_forward(m, x)[0]
        res['torch_ms'] = round(timed(torch_step, a.steps, a.warmup), 3)
        res['max_abs_diff_logits'] = float((yb - yt).abs().max())
        res['speedup'] = round(res['torch_ms'] / res['build_ms'], 2)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
