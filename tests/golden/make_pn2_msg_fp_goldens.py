#!/usr/bin/env python3
"""Generate tests/golden/pn2_msg_fp.npz by RUNNING THE REFERENCE's PointNetSetAbstractionMsg, both
PointNetFeaturePropagation classes and TransitionUp (build container only, CPU).

Usage (from the repo root, ~1 min):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pn2_msg_fp_goldens.py

Uses make_goldens.py's set-up (stub modules, the 'cuda' -> 'cpu' redirect, the reference on sys.path).  Inputs, the case
table, the composer of the six-module network and the forward + backward runner come from tests/pn2_msg_fp_cases.py, which
the tests share; here they are applied to the reference classes.  The fixture holds seeds, index lists (int16), small
outputs, seeded subsets of wide outputs, norms, probe dots and name lists -- no clouds, no weights.

  1. operators: ball-query lists for radii (0.1, 0.2, 0.4) / nsample (32, 64, 128), N = 1024, S = 512; 3-NN lists in the
     expanded and the direct distance form for (N, S) = (1024, 256), (1024, 64), (256, 4), (64, 3), fp32 and fp64; the
     interpolation of D2 = 16 features, fp32 and fp64, and the reference's own max-abs fp32-vs-fp64 deviation;
  2. every case of pn2_msg_fp_cases.CASES in train and in eval mode, fp32 and fp64;
  3. the composed network (N = 1024), train mode fp32 and fp64, eval mode fp32.
The preconditions a test would otherwise have to excuse are asserted here: no exact distance tie among a query's four
nearest, fp32 and fp64 3-NN lists equal, every |d + 1e-8| > 1e-9, no pair within 1e-6 relative of a squared radius, no
empty ball, everything finite."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as MG                 # noqa: E402  (stubs, cuda -> cpu redirect, reference on sys.path)

import model.pointnet2_utils as r_p2      # noqa: E402  (reference)
import model.PTran_utils as r_ptu         # noqa: E402
import model.Ptran_model as r_PT          # noqa: E402

import pn2_msg_fp_cases as C              # noqa: E402

RADII, NSAMPLE = (0.1, 0.2, 0.4), (32, 64, 128)
NN_CASES = ((1024, 256, 71), (1024, 64, 72), (256, 4, 76), (64, 3, 77))
NET_SEED = 95


class Ref:
    Msg, FP, FPDirect, TU = r_p2.PointNetSetAbstractionMsg, r_p2.PointNetFeaturePropagation, r_ptu.PointNetFeaturePropagation, \
        r_PT.TransitionUp

    @staticmethod
    def All(in_channel, mlp):
        return r_p2.PointNetSetAbstraction(None, None, None, in_channel, mlp, group_all=True)


def finite(t, what):
    assert bool(torch.isfinite(torch.as_tensor(t)).all()), what + ': not finite'


def operators(out):
    rows = C.clouds(C.BQ_SEED, 1024).permute(0, 2, 1).contiguous()
    torch.manual_seed(C.BQ_SEED + 1)
    fps = r_p2.farthest_point_sample(rows, 512)
    cen = r_p2.index_points(rows, fps)
    d = r_p2.square_distance(cen, rows)
    out['bq_fps'] = fps
    for i, (r, K) in enumerate(zip(RADII, NSAMPLE)):
        assert not bool(((d - r ** 2).abs() <= 1e-6 * r ** 2).any()), 'a pair lies within 1e-6 relative of r^2 = %g' % r ** 2
        idx = r_p2.query_ball_point(r, K, rows, cen)
        assert int(idx.max()) < 1024, 'empty ball at radius %g' % r
        if K <= 64:
            out['bq_idx%d' % i] = idx
        else:                      # too large to store: a hash of the whole list, and the lists of a subset of the queries
            out['bq_idx%d_sha256' % i] = np.array([C.list_hash(idx)])
            out['bq_idx%d_sub' % i] = torch.gather(idx, 1, C.subset(512, C.BQ_SEED).unsqueeze(-1).expand(-1, -1, K))
        print('ball query r=%.1f: mean hits %.1f, %d groups overflow %d' % (r, float((d <= r ** 2).sum(-1).float().mean()),
                                                                           int(((d <= r ** 2).sum(-1) > K).sum()), K))
    for c, (N, S, seed) in enumerate(NN_CASES):
        xyz1 = C.clouds(seed, N)
        torch.manual_seed(seed + 1)
        fps = r_p2.farthest_point_sample(xyz1.permute(0, 2, 1), S)
        xyz2 = r_p2.index_points(xyz1.permute(0, 2, 1), fps).permute(0, 2, 1).contiguous()
        p2 = C.feats(seed, 16, S, 'p2')
        ids = C.subset(N, seed)
        out['nn%d_meta' % c] = np.array([N, S, seed])
        out['nn%d_fps' % c] = fps
        for form, mod in (('exp', r_p2), ('dir', r_ptu)):
            pre = 'nn%d_%s_' % (c, form)
            lists = []
            for dt in (torch.float32, torch.float64):
                dd, ii = mod.square_distance(xyz1.permute(0, 2, 1).to(dt), xyz2.permute(0, 2, 1).to(dt)).sort(dim=-1)
                if S >= 4 and dt == torch.float32:
                    assert bool((dd[:, :, 1:4] != dd[:, :, 0:3]).all()), pre + 'an exact distance tie among the four nearest'
                elif dt == torch.float32:
                    assert bool((dd[:, :, 1:3] != dd[:, :, 0:2]).all()), pre + 'an exact distance tie'
                assert float((dd[:, :, :3] + 1e-8).abs().min()) > 1e-9, pre + 'a |d + 1e-8| below 1e-9'
                lists.append(ii[:, :, :3])
                if dt == torch.float32:
                    print('%s self-distance < 0: %d, min |d + 1e-8| %.3g' % (pre, int((dd[:, :, 0] < 0).sum()),
                                                                            float((dd[:, :, :3] + 1e-8).abs().min())))
            assert torch.equal(lists[0], lists[1]), pre + 'fp32 and fp64 3-NN lists differ'
            out[pre + 'idx32'], out[pre + 'idx64'] = lists
            fp = mod.PointNetFeaturePropagation(-1, [])
            y32 = fp(xyz1, xyz2, None, p2)
            y64 = fp(xyz1.double(), xyz2.double(), None, p2.double())
            finite(y32, pre + 'interpolation')
            pr = C.probe(y32.shape, 'interp')
            out[pre + 'sub32'], out[pre + 'sub64'] = C.take_points(y32, ids), C.take_points(y64, ids)
            out[pre + 'stat32'] = np.array([y32.double().norm().item(), (y32.double() * pr.double()).sum().item()])
            out[pre + 'stat64'] = np.array([y64.norm().item(), (y64 * pr.double()).sum().item()])
            out[pre + 'dev'] = (y32.double() - y64).abs().max().item()
            print('%s reference interpolation fp32 vs fp64: max abs %.2e' % (pre, out[pre + 'dev']))


def record(out, pre, r32, r64, ids, full64=True):
    """ids: None (keep the whole output) or the [B,n] subset of points; r64 None: an fp32-only record; full64 False: of the
    fp64 run only norms, probe dots and the loss are kept."""
    finite(r32['out'], pre + 'output')
    keep = (lambda t: t) if ids is None else (lambda t: C.take_points(t, ids))
    o32 = r32['out']
    pr = C.probe(o32.shape, 'stat')
    out[pre + 'out32'] = keep(o32)
    out[pre + 'stat32'] = np.array([o32.double().norm().item(), (o32.double() * pr.double()).sum().item()])
    out[pre + 'loss32'] = r32['loss']
    if r32['aux'] is not None:
        out[pre + 'aux'] = r32['aux']
    out[pre + 'bn_names'] = np.array(r32['bn_names'])
    out[pre + 'bn_sum'] = np.array(r32['bn_sum'])
    if 'grad_names' in r32:
        out[pre + 'grad_names'] = np.array(r32['grad_names'])
        out[pre + 'grad_norm32'], out[pre + 'grad_dot32'] = np.array(r32['grad_norm']), np.array(r32['grad_dot'])
        finite(out[pre + 'grad_norm32'], pre + 'gradients')
    if r64 is not None:
        o64 = r64['out']
        if full64:
            out[pre + 'out64'] = keep(o64)
        out[pre + 'stat64'] = np.array([o64.norm().item(), (o64 * pr.double()).sum().item()])
        out[pre + 'loss64'] = r64['loss']
        if 'grad_names' in r64:
            assert r64['grad_names'] == r32['grad_names']
            out[pre + 'grad_norm64'], out[pre + 'grad_dot64'] = np.array(r64['grad_norm']), np.array(r64['grad_dot'])
        if r32['aux'] is not None:
            assert torch.equal(r32['aux'].double(), r64['aux']), pre + 'fp32 and fp64 runs sampled different points'


def classes(out):
    for name, (kind, _, seed) in C.CASES.items():
        args, gix = C.case_inputs(name)
        net = C.build(Ref, name)
        sd = net.state_dict()
        out[name + '_keys'] = np.array(list(sd.keys()))
        out[name + '_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
        if name == 'fp_s2':
            try:
                C.run(net.train(), args, gix, seed)
            except RuntimeError as e:
                out['fp_s2_error'] = np.array([str(e)[:120]])
                print('fp_s2: the reference fails as expected:', str(e)[:80])
                continue
            raise AssertionError('the reference accepted S = 2')
        for mode in ('train', 'eval'):
            n32 = C.build(Ref, name).train(mode == 'train')
            n64 = C.build(Ref, name).double().train(mode == 'train')
            r32 = C.run(n32, args, gix, seed)
            r64 = C.run(n64, args, gix, seed, dtype=torch.float64)
            for r in (r32, r64):
                r['out'] = C.case_out(name, r['out'])
            record(out, '%s_%s_' % (name, mode), r32, r64, C.case_ids(name, r32['out'].shape[2]), full64=mode == 'train')
        print('%-10s ok' % name)


def network(out):
    xyz = C.clouds(NET_SEED, 1024)
    ids = C.subset(1024, NET_SEED)
    for mode in ('train', 'eval'):
        n32 = C.SegNet(Ref)
        C.load_seeded(n32, NET_SEED)
        n32.train(mode == 'train')
        r32 = C.run(n32, [xyz], [], NET_SEED, loss_kind='square')
        r64 = None
        if mode == 'train':
            n64 = C.SegNet(Ref)
            C.load_seeded(n64, NET_SEED)
            r64 = C.run(n64.double().train(), [xyz], [], NET_SEED, dtype=torch.float64, loss_kind='square')
            sd = n32.state_dict()
            out['net_keys'] = np.array(list(sd.keys()))
            out['net_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
            print('composed network: %d parameters, loss %.6f (fp64 %.6f)' % (sum(p.numel() for p in n32.parameters()), r32['loss'],
                                                                           r64['loss']))
        record(out, 'net_%s_' % mode, r32, r64, ids)


if __name__ == '__main__':
    torch.set_num_threads(8)
    out = {}
    operators(out)
    classes(out)
    network(out)
    MG.save('pn2_msg_fp.npz', **out)
    size = os.path.getsize(os.path.join(HERE, 'pn2_msg_fp.npz'))
    assert size < 1000 * 1000, 'the fixture has %d bytes' % size
