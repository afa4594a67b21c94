"""Kernel time of the reverse-list build (sug_knn_reverse) on destination patterns of low and high hubness.
Cases: 64 clouds x 1024 points, k = 20 (the EdgeConv backward's shape) with kNN graphs in xyz and in feature space,
uniformly random destinations, one destination listed by every entry, three destinations with a third of the entries
each; and the interpolation shape (64 clouds, 3072 entries into 64 destinations, passed as N = 64, k = 48).
Every case is captured REPS times into one graph and the replay is timed, so that the figure is the kernel's time and
not the launch rate of the Python caller.
usage: python tools/bench_reverse.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sug_amd import ops

REPS, ROUNDS = 20, 5
torch.manual_seed(0)
B, N, K = 64, 1024, 20
dev = 'cuda'


def rand(n, k):
    return torch.randint(0, n, (B, n, k), dtype=torch.int32, device=dev)


cases = {
    'knn xyz': ops.knn(torch.rand(B, N, 3, device=dev), K),
    'knn feat64': ops.knn(torch.randn(B, N, 64, device=dev) * 0.3 + torch.randn(B, 1, 64, device=dev), K),
    'uniform': rand(N, K),
    'hub: one destination': torch.full((B, N, K), 7, dtype=torch.int32, device=dev),
    'hub: three destinations': (torch.arange(N * K, device=dev) * 3 // (N * K)).to(torch.int32).mul(341).reshape(1, N, K).repeat(B, 1, 1),
    'interp 3072 -> 64': rand(64, 48),
}
print('%-26s %10s %10s %10s   %s' % ('case', 'us median', 'us min', 'us max', 'list length max / share > 32'))
for name, idx in cases.items():
    idx = idx.contiguous()
    off, _ = ops.knn_reverse(idx)
    cnt = off[:, 1:] - off[:, :-1]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.knn_reverse(idx)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            ops.knn_reverse(idx)
    graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(ROUNDS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        graph.replay()
        t1.record()
        torch.cuda.synchronize()
        us.append(t0.elapsed_time(t1) * 1000.0 / REPS)
    us.sort()
    print('%-26s %10.2f %10.2f %10.2f   %d / %.3f' % (name, us[ROUNDS // 2], us[0], us[-1], int(cnt.max()),
                                                      float((cnt > 32).float().mean())))
