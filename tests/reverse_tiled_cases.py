"""Cases and CPU reference of the tiled reverse-list build (sug_reverse_lists_tiled / ops.reverse_lists_tiled), shared by
tests/test_reverse_tiled_host.py and tests/test_gpu_reverse_tiled.py.

The contract is that of sug_reverse_lists_build (tests/reverse_lists_cases.py): per cloud, rev_ent is
torch.argsort(idx, stable=True) restricted to the entries whose destination lies in [0, N), rev_off the exclusive prefix
of the destinations' counts, rev_off[:, N] the number of valid entries.  reference() here takes any tensor."""
import functools

import torch

# name -> (B, E, N, tile, pattern, share of invalid entries): each shape is the smallest at which the named part of the
# tiled kernel can go wrong (tile = 1024 entries unless said otherwise)
CASES = {
    'one_entry': (1, 1, 1, 1024, 'uniform', 0.0),
    'partial_tile_few_dest': (2, 700, 7, 1024, 'uniform', 0.0),       # one partial tile, fewer destinations than lanes
    'whole_tiles': (2, 3072, 96, 1024, 'uniform', 0.0),
    'ragged': (3, 3000, 1000, 1024, 'uniform', 0.0),                  # partial last tile, ranges that do not divide N
    'last_tile_of_one': (2, 2049, 64, 1024, 'uniform', 0.0),
    'one': (2, 5000, 300, 1024, 'one', 0.0),                          # one list across five tiles, one range holds all
    'gap': (2, 3072, 50, 1024, 'gap', 0.0),                           # the cursor carries over a tile without the list
    'blocks': (2, 4096, 512, 1024, 'blocks', 0.0),                    # ranges see tiles with no entry of theirs
    'unlisted': (3, 3000, 1000, 1024, 'unlisted', 0.0),               # odd destinations and the upper third empty
    'invalid': (3, 3000, 1000, 1024, 'uniform', 0.1),
    'invalid_cloud': (2, 2500, 64, 1024, 'invalid_cloud', 0.0),       # cloud 1: rev_off all zero, rev_ent untouched
    'more_dest_than_entries': (2, 2048, 4096, 1024, 'uniform', 0.0),
    'hubs': (5, 20000, 1000, 2048, 'hubs', 0.0),                      # the kNN shape, through a second tile size
}
TILE_SWEEP = ('ragged', 'gap', 'hubs')                                # run at tile 1024, 2048 and 0: identical arrays

# the sizes the LDS-resident build refuses, at the library's tile (0)
REAL = {
    'n2048_k20-uniform': (2, 40960, 2048, 0, 'uniform', 0.0),
    'n2048_k20-hubs': (2, 40960, 2048, 0, 'hubs', 0.0),
    'n2048_k33-uniform': (2, 67584, 2048, 0, 'uniform', 0.0),         # crosses 65 536 entries
    'n2048_k33-one': (2, 67584, 2048, 0, 'one', 0.0),
    'lists_of_768': (1, 49152, 64, 0, 'equal', 0.0),
    'n_at_the_limit': (1, 70000, 32768, 0, 'uniform', 0.0),
}
ALL = dict(CASES, **REAL)


def draw(B, E, N, pattern, invalid, seed):
    """idx [B, E] int32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if pattern == 'uniform':
        idx = torch.randint(0, N, (B, E), generator=g, dtype=torch.int32)
    elif pattern == 'hubs':       # E = N * k: three destinations with a third of a column each, one with N/2 entries
        k = E // N
        assert k * N == E and k >= 2
        idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32)
        idx[:, :, 0] = torch.randint(0, min(3, N), (B, N), generator=g, dtype=torch.int32)
        idx[:, : N // 2, 1] = N - 1
        idx = idx.reshape(B, E)
    elif pattern == 'one':        # one destination listed by every entry
        idx = torch.full((B, E), N // 3, dtype=torch.int32)
    elif pattern == 'unlisted':   # destinations nobody lists: every odd one and the whole upper third
        idx = torch.randint(0, max(1, N // 3), (B, E), generator=g, dtype=torch.int32) * 2
    elif pattern == 'gap':        # destination N // 2: in the first and the third 1024 entries, not in the second
        d = N // 2
        idx = torch.randint(0, N - 1, (B, E), generator=g, dtype=torch.int32)
        idx += (idx >= d).int()
        idx[:, 5:1000:7] = d
        idx[:, 2048 + 3:2048 + 900:11] = d
    elif pattern == 'blocks':     # the t-th 1024 entries list only the t-th quarter of the destinations
        q = N // 4
        idx = torch.randint(0, q, (B, E), generator=g, dtype=torch.int32) + (torch.arange(E) // 1024 % 4).int() * q
    elif pattern == 'invalid_cloud':
        idx = torch.randint(0, N, (B, E), generator=g, dtype=torch.int32)
        idx[1] = torch.tensor([-1, N, N + 5], dtype=torch.int32)[torch.randint(0, 3, (E,), generator=g)]
    elif pattern == 'equal':      # every destination E / N times, in random order
        assert E % N == 0
        idx = torch.stack([(torch.randperm(E, generator=g) % N).int() for _ in range(B)])
    else:
        raise KeyError(pattern)
    if invalid:
        bad = torch.rand(B, E, generator=g) < invalid
        what = torch.tensor([-1, N, N + 5], dtype=torch.int32)[torch.randint(0, 3, (B, E), generator=g)]
        idx = torch.where(bad, what, idx)
    return idx


@functools.lru_cache(maxsize=None)
def make(case):
    """idx [B, E] int32 on the CPU (seeded by the case's name; cached: treat it as read-only)."""
    B, E, N, _, pattern, invalid = ALL[case]
    return draw(B, E, N, pattern, invalid, sum(map(ord, case)))


def reference(idx, N):
    """(rev_off [B, N+1] int64, rev_ent [B, E] int64 of which row b's first rev_off[b, N] entries count) of any
    idx [B, E]: the stable argsort, invalid entries behind all others."""
    B, E = idx.shape
    flat = idx.cpu().long()
    key = torch.where((flat >= 0) & (flat < N), flat, torch.full_like(flat, N))
    ent = torch.argsort(key, dim=1, stable=True)
    counts = torch.zeros(B, N + 1, dtype=torch.long).scatter_add_(1, key, torch.ones_like(key))
    off = torch.cat((torch.zeros(B, 1, dtype=torch.long), counts[:, :N].cumsum(1)), 1)
    return off, ent


@functools.lru_cache(maxsize=None)
def case_reference(case):
    return reference(make(case), ALL[case][2])
