"""Cases and CPU reference of the reverse-list build (sug_reverse_lists_build / ops.reverse_lists), shared by
tests/test_reverse_lists_host.py and tests/test_gpu_reverse_lists.py.

The reference: per cloud, rev_ent is torch.argsort(idx, stable=True) restricted to the entries whose destination lies
in [0, N), rev_off the exclusive prefix of the destinations' counts, rev_off[:, N] the number of valid entries."""
import functools

import torch

LDS_LIMIT = 160 * 1024


def lds_bytes(B, E, N):
    """(bytes, destination ranges per cloud): the formula of sug_reverse_lists_lds_bytes (sug_amd/csrc/knn.hip), restated;
    test_reverse_lists_host.py holds it against the library's answers on both sides of the limit."""
    rs = 1
    while rs < 8 and B * rs < 256 and N // (rs * 2) >= 64:
        rs *= 2
    nr = (N + rs - 1) // rs
    return 4 * (2 * nr + 32 + E), rs


def max_entries(B, N):
    """The largest E the formula accepts for B clouds and N destinations."""
    E = LDS_LIMIT // 4 - 32 - 2 * ((N + lds_bytes(B, 1, N)[1] - 1) // lds_bytes(B, 1, N)[1])
    assert lds_bytes(B, E, N)[0] <= LDS_LIMIT < lds_bytes(B, E + 1, N)[0]
    return E


# (B, E, N, k): k is the neighbour count when E = N * k (the case then also runs through ops.knn_reverse), else None
SHAPES = {
    'one_entry': (1, 1, 1, 1),
    'one_dest': (2, 20, 1, 20),                  # every entry lists one destination: a list longer than a half-wave
    'few_dest': (3, 140, 7, 20),                 # fewer destinations than lanes
    'one_range': (2, 96 * 20, 96, 20),
    'ragged_ranges': (5, 1000 * 20, 1000, 20),   # ranges that do not divide N, a partial last range
    'n512': (40, 512 * 20, 512, 20),
    'interp_odd': (2, 3 * 257, 64, None),        # the interpolation shape: lists longer than 32
    'interp': (2, 3 * 1024, 64, 48),
    'sparse': (2, 64 * 32, 2048, 1),             # more destinations than entries per range: many empty lists
    'bench': (64, 1024 * 20, 1024, 20),
    'max_n512': (2, max_entries(2, 512), 512, None),
    'max_n2048': (2, max_entries(2, 2048), 2048, None),
}

# name -> (shape, pattern, share of invalid entries)
CASES = {s + '-uniform': (s, 'uniform', 0.0) for s in SHAPES}
for _s in ('one_range', 'ragged_ranges', 'n512'):                       # the benchmark-shaped ones, small
    for _p in ('hubs', 'one', 'unlisted'):
        CASES['%s-%s' % (_s, _p)] = (_s, _p, 0.0)
CASES['max_n512-one'] = ('max_n512', 'one', 0.0)                        # the longest run a thread can own
for _s in ('few_dest', 'ragged_ranges', 'interp'):
    CASES[_s + '-invalid'] = (_s, 'uniform', 0.1)

SMALL = [c for c, (s, _, _) in CASES.items() if SHAPES[s][0] * SHAPES[s][1] <= 8192]


@functools.lru_cache(maxsize=None)
def make(case):
    """idx [B, E] int32 on the CPU (seeded by the case's name; cached: treat it as read-only)."""
    shape, pattern, invalid = CASES[case]
    B, E, N, k = SHAPES[shape]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    if pattern == 'uniform':
        idx = torch.randint(0, N, (B, E), generator=g, dtype=torch.int32)
    elif pattern == 'hubs':       # three destinations with a third of a column each, one with N/2 (test_knn_reverse_lists_full)
        idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32)
        idx[:, :, 0] = torch.randint(0, min(3, N), (B, N), generator=g, dtype=torch.int32)
        idx[:, : N // 2, 1] = N - 1
        idx = idx.reshape(B, E)
    elif pattern == 'one':        # one destination listed by every entry
        idx = torch.full((B, E), N // 3, dtype=torch.int32)
    elif pattern == 'unlisted':   # destinations nobody lists: every odd one and the whole upper third
        idx = torch.randint(0, max(1, N // 3), (B, E), generator=g, dtype=torch.int32) * 2
    else:
        raise KeyError(pattern)
    if invalid:
        bad = torch.rand(B, E, generator=g) < invalid
        what = torch.tensor([-1, N, N + 5], dtype=torch.int32)[torch.randint(0, 3, (B, E), generator=g)]
        idx = torch.where(bad, what, idx)
    return idx


@functools.lru_cache(maxsize=None)
def reference(case):
    """(rev_off [B, N+1] int64, rev_ent [B, E] int64 of which row b's first rev_off[b, N] entries count)."""
    idx = make(case)
    N = SHAPES[CASES[case][0]][2]
    B, E = idx.shape
    flat = idx.long()
    key = torch.where((flat >= 0) & (flat < N), flat, torch.full_like(flat, N))      # invalid entries behind all others
    ent = torch.argsort(key, dim=1, stable=True)
    counts = torch.zeros(B, N + 1, dtype=torch.long).scatter_add_(1, key, torch.ones_like(key))
    off = torch.cat((torch.zeros(B, 1, dtype=torch.long), counts[:, :N].cumsum(1)), 1)
    return off, ent
