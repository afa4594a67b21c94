#!/usr/bin/env python3
"""Part segmentation: the three new pieces against their composed forms IN THE SAME TREE, on the same GPU, alternated in one
process, device events, the median of rounds with every round reported (the spread is max - min of the rounds).

  point_ce   forward + backward at M = 32768, C = 50: ops.point_ce (with the arg-max) | F.cross_entropy + argmax
  part_iou   B = 16, N = 2048, C = 50, K = 16: ops.part_iou_accumulate | the same protocol in torch ops on the device plus
             the per-batch host read it needs (its shape IoUs are averaged on the host)
  seg_step   one SegStep at B = 16, N = 2048 | the same model with F.cross_entropy + argmax and torch.optim.Adam

    python tools/bench_seg.py [--iters 50] [--warmup 5] [--out profiles/seg_bench.json] [--skip-step]

point_ce is reported three ways: eager calls under device events (the larger of host and device time), the host time alone,
and the device time alone (both paths replayed from a captured graph).
Launches are counted with torch.profiler over one call of each path (kernel events; null where the profiler is unavailable).
Algorithmic bytes (each input once, each output once): point_ce forward M(4C + 8) + M(8 + 4) (logits, labels; lse pair, pred),
backward M(4C + 8 + 8) + 4MC; part_iou B N (4C + 8)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

M, C = 32768, 50
B, N, K = 16, 2048, 16
# ShapeNet-Part: 16 categories over 50 parts
PART_COUNT = [4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3]
PART_FIRST = [sum(PART_COUNT[:k]) for k in range(K)]
ROUNDS = 5


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def launches(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception:       # noqa: BLE001 -- a count is a side note of the timing
        return None


def host_us(fn, iters):
    """Host time of one call (perf_counter around `iters` calls, the device drained before and after, not in between)."""
    import time
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    dt = time.perf_counter() - t
    torch.cuda.synchronize()
    return round(dt / iters * 1e6, 2)


def graph_us(fn, iters):
    """Device time of one call: captured into a hipGraph and replayed (no host work between the launches); None where the
    capture is refused."""
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        v = sorted(event_ms(graph.replay, iters) for _ in range(ROUNDS))
        return round(v[len(v) // 2] * 1e3, 2)
    except Exception:       # noqa: BLE001
        return None


def alternate(paths, a):
    for f in paths.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    per = max(a.iters // ROUNDS, 1)
    ms = {k: [] for k in paths}
    for _ in range(ROUNDS):                       # alternated: both see the same clocks and cache state drift
        for k, f in paths.items():
            ms[k].append(event_ms(f, per))
    out = {'iters_per_path': ROUNDS * per}
    for k, v in ms.items():
        out[k + '_us'] = round(sorted(v)[len(v) // 2] * 1e3, 2)
        out[k + '_us_rounds'] = [round(x * 1e3, 2) for x in v]
        out[k + '_us_spread'] = round((max(v) - min(v)) * 1e3, 2)
        out[k + '_launches'] = launches(paths[k])
    return out


def bench_point_ce(a):
    from sug_amd import ops
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(M, C, generator=g) * 3).cuda().requires_grad_(True)
    lab = torch.randint(0, C, (M,), generator=g).cuda()

    def fused():
        loss, pred = ops.point_ce(z, lab, want_pred=True)
        torch.autograd.grad(loss, z)

    def composed():
        loss = F.cross_entropy(z, lab)
        z.detach().argmax(dim=1)
        torch.autograd.grad(loss, z)
    res = alternate({'fused': fused, 'composed': composed}, a)
    res['_paths'] = (fused, composed)
    # where an eager call's time goes: the host's share of the forward alone and of forward + backward (the backward of a
    # Python autograd Function runs on autograd's device thread, which has to be woken and to take the GIL)
    res['fused_forward_host_us'] = host_us(lambda: ops.point_ce(z, lab, want_pred=True), 200)
    res['fused_host_us'] = host_us(fused, 200)
    res['composed_host_us'] = host_us(composed, 200)
    res.update(M=M, C=C, algorithmic_MB=round((M * (4 * C + 8) + M * 12 + M * (4 * C + 16) + 4 * M * C) / 1e6, 2),
               speedup=round(res['composed_us'] / res['fused_us'], 2))
    return res


def torch_part_iou(logits, label, category, first, count, maxp):
    """The protocol in torch ops on the device: masked arg-max over each cloud's range, one-hot counts per part slot, the
    shape IoUs; then the host read a per-batch meter needs."""
    Bq, Nq, Cq = logits.shape
    f, n = first[category], count[category]                                    # [B]
    slot = torch.arange(maxp, device=logits.device)
    cols = (f.view(Bq, 1) + slot.view(1, -1)).clamp(max=Cq - 1)                 # [B, maxp]
    valid = slot.view(1, -1) < n.view(Bq, 1)
    sub = torch.gather(logits, 2, cols.view(Bq, 1, maxp).expand(Bq, Nq, maxp)).masked_fill(~valid.view(Bq, 1, maxp), float('-inf'))
    pred = sub.argmax(dim=2)
    lab = label - f.view(Bq, 1)
    p1, l1 = F.one_hot(pred, maxp).bool(), F.one_hot(lab, maxp).bool()
    inter = (p1 & l1).sum(1).double()
    union = (p1 | l1).sum(1).double()
    iou = torch.where(union == 0, torch.ones_like(union), inter / union.clamp(min=1))
    shape_iou = (iou * valid).sum(1) / n
    return torch.cat([shape_iou, (pred == lab).sum(1).double()]).cpu()          # the per-batch host read


def bench_part_iou(a):
    from sug_amd import ops
    g = torch.Generator().manual_seed(1)
    cat = torch.randint(0, K, (B,), generator=g)
    first, count = torch.tensor(PART_FIRST), torch.tensor(PART_COUNT)
    lab = torch.stack([first[k] + torch.randint(0, int(count[k]), (N,), generator=g) for k in cat])
    z = torch.randn(B, N, C, generator=g).cuda()
    cat, lab = cat.cuda(), lab.cuda()
    fd, cd = first.cuda(), count.cuda()
    state = ops.part_iou_state('cuda')

    def fused():
        ops.part_iou_accumulate(z, lab, cat, PART_FIRST, PART_COUNT, state)

    def composed():
        torch_part_iou(z, lab, cat, fd, cd, max(PART_COUNT))
    res = alternate({'fused': fused, 'composed': composed}, a)
    # the two forms agree on this batch
    st = ops.part_iou_state('cuda')
    ops.part_iou_accumulate(z, lab, cat, PART_FIRST, PART_COUNT, st)
    f = ops.part_iou_state_fields(st)
    ref = torch_part_iou(z, lab, cat, fd, cd, max(PART_COUNT))
    res.update(B=B, N=N, C=C, K=K, algorithmic_MB=round(B * N * (4 * C + 8) / 1e6, 2),
               speedup=round(res['composed_us'] / res['fused_us'], 2),
               shape_iou_sum_diff=abs(float(f['cat_iou'].sum()) - float(ref[:B].sum())),
               correct_equal=int(f['correct']) == int(ref[B:].sum()))
    return res


def bench_step(a):
    import pn2_msg_fp_cases as PC
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    from sug_amd.seg_step import SegStep
    pts = PC.clouds(0, N, batch=B).cuda()
    g = torch.Generator().manual_seed(2)
    cat = torch.randint(0, K, (B,), generator=g).cuda()
    lab = torch.randint(0, C, (B, N), generator=g).cuda()
    nets = []
    for _ in range(2):
        net = Pointnet2PartSeg()
        PC.load_seeded(net, 0)
        nets.append(net.cuda().train())
    step = SegStep(nets[0])
    opt = torch.optim.Adam(nets[1].parameters(), lr=1e-3, weight_decay=1e-4)
    books = torch.zeros(3, dtype=torch.float64, device='cuda')

    def fused():
        step.step(pts, cat, lab)

    def composed():
        logits, _ = nets[1](pts, cat)
        flat = logits.reshape(-1, C)
        loss = F.cross_entropy(flat, lab.reshape(-1))
        with torch.no_grad():
            books[0:1].add_(loss.detach().double().reshape(1), alpha=B * N)
            books[2:].add_((flat.argmax(dim=1) == lab.reshape(-1)).sum())
        loss.backward()
        opt.step()
        opt.zero_grad()
    res = alternate({'fused': fused, 'composed': composed}, a)
    res = {k.replace('_us', '_ms'): (round(v / 1e3, 3) if isinstance(v, float) else
                                     [round(x / 1e3, 3) for x in v] if isinstance(v, list) else v) for k, v in res.items()}
    res.update(B=B, N=N, speedup=round(res['composed_ms'] / res['fused_ms'], 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'workload': 'part segmentation: per-point cross entropy, part-IoU books, SegStep -- fused vs composed, same tree',
           'point_ce': bench_point_ce(a), 'part_iou': bench_part_iou(a)}
    if not a.skip_step:
        a.iters = max(a.iters // 2, ROUNDS)
        res['seg_step'] = bench_step(a)
    # the point_ce calls above are bound by the host (a handful of launches of a few microseconds each): the same calls
    # replayed from a captured graph give the device's share (last: a refused capture ends nothing else)
    fused, composed = res['point_ce'].pop('_paths')
    res['point_ce']['fused_graph_replay_us'] = graph_us(fused, 20)
    res['point_ce']['composed_graph_replay_us'] = graph_us(composed, 20)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
