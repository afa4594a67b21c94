"""Cases and CPU restatements for the ChamferDistance op (sug_chamfer_nn / sug_chamfer_nn_bwd): shared by
test_chamfer_host.py (no GPU) and test_gpu_chamfer.py.  Everything is generated from seeds."""
import functools

import torch

U = 2.0 ** -24            # unit roundoff of fp32

# (B, N, M): a lane without a candidate (M < 4), tails of the unrolled candidate loop (M = 7, 9), a partial last workgroup
# (N = 65, 257), more than one workgroup per cloud (N = 257, 1024), N != M, more than one LDS tile and the size limit (5000)
SHAPES = [(1, 1, 1), (2, 1, 7), (2, 3, 2), (3, 65, 9), (3, 257, 64), (2, 1024, 1021), (1, 5000, 3), (1, 3, 5000)]


def random_clouds(B, N, M, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + M)
    return torch.rand(B, N, 3, generator=g) * 2 - 1, torch.rand(B, M, 3, generator=g) * 2 - 1


def _grid_cloud(B, n, g):
    """n points with coordinates k / 64 in [-1, 1], every point of a pool of ceil(n / 3) present two or three times (all of
    them at least twice once n >= 2), at positions drawn by a permutation: whatever point is nearest, an exact copy of it
    sits at another index, at another residue mod 8 for most of them."""
    pool = (n + 2) // 3
    pts = torch.randint(-64, 65, (B, pool, 3), generator=g).float() / 64
    out = pts[:, torch.arange(n) % pool]
    return torch.stack([out[i, torch.randperm(n, generator=g)] for i in range(B)])


def grid_clouds(B, N, M, seed=0):
    g = torch.Generator().manual_seed(2000 * seed + 7 * N + M)
    return _grid_cloud(B, N, g), _grid_cloud(B, M, g)


def hub_clouds(N=65, M=1021, seed=0):
    """Two pairs; one point of `a` (index 0 in pair 0, index 37 in pair 1) is the nearest of ALL M points of b, the other
    points of a lie far away: M contributions to one target of ga, none to the others."""
    g = torch.Generator().manual_seed(3000 + seed)
    a = torch.rand(2, N, 3, generator=g) + 50.0
    b = torch.rand(2, M, 3, generator=g) * 2 - 1
    a[0, 0] = torch.tensor([0.1, -0.2, 0.05])
    a[1, 37] = torch.tensor([-0.3, 0.15, 0.2])
    return a, b


def pair_sq_dist_fp32(a, b):
    """[B,N,M] squared distances in the kernel's operation order, fp32, every operation rounded once."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    dx = a[:, :, None, :] - b[:, None, :, :]
    d0, d1, d2 = dx[..., 0], dx[..., 1], dx[..., 2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def _min_lowest(d):
    """min over the last dimension and the LOWEST index attaining it (no reliance on how torch.min / argmin break ties)."""
    n = d.shape[-1]
    m = d.min(dim=-1).values
    idx = torch.where(d == m[..., None], torch.arange(n), torch.tensor(n)).min(dim=-1).values
    return m, idx


def nn_fp32(a, b):
    """Restatement (a): (dist1 [B,N], dist2 [B,M], idx1, idx2 int64) on the CPU in fp32, bit for bit what the kernel computes."""
    d = pair_sq_dist_fp32(a, b)
    dist1, idx1 = _min_lowest(d)
    dist2, idx2 = _min_lowest(d.transpose(1, 2))
    return dist1, dist2, idx1, idx2


def tie_counts(a, b):
    """Number of query points of each direction whose minimum is attained by more than one candidate."""
    d = pair_sq_dist_fp32(a, b)
    t1 = ((d == d.min(dim=2, keepdim=True).values).sum(2) > 1).sum().item()
    t2 = ((d == d.min(dim=1, keepdim=True).values).sum(1) > 1).sum().item()
    return t1, t2


def grads_fp64(a, b, idx1, idx2, g1, g2):
    """Restatement (b), fp64, gathering by the GIVEN indices: dist1 [B,N], dist2 [B,M] and, for upstream g1, g2,
    ga_i = 2 g1_i (a_i - b_idx1[i]) + sum_{j: idx2[j] = i} 2 g2_j (a_i - b_j) and the symmetric gb; per gradient component also
    K (the number of contributions arriving from the other cloud's points) and S (the sum of |term| over all its terms)."""
    a, b, g1, g2 = (t.detach().cpu().double() for t in (a, b, g1, g2))
    idx1, idx2 = idx1.detach().cpu().long(), idx2.detach().cpu().long()
    e1 = idx1[..., None].expand(-1, -1, 3)
    e2 = idx2[..., None].expand(-1, -1, 3)
    da = a - torch.gather(b, 1, e1)                    # a_i - b_idx1[i]
    db = b - torch.gather(a, 1, e2)                    # b_j - a_idx2[j]
    t1 = 2 * g1[..., None] * da                        # own terms of ga; their negatives arrive at gb[idx1]
    t2 = 2 * g2[..., None] * db
    ga = t1 + torch.zeros_like(a).scatter_add_(1, e2, -t2)
    gb = t2 + torch.zeros_like(b).scatter_add_(1, e1, -t1)
    Sa = t1.abs() + torch.zeros_like(a).scatter_add_(1, e2, t2.abs())
    Sb = t2.abs() + torch.zeros_like(b).scatter_add_(1, e1, t1.abs())
    Ka = torch.zeros_like(a).scatter_add_(1, e2, torch.ones_like(b))
    Kb = torch.zeros_like(b).scatter_add_(1, e1, torch.ones_like(a))
    return dict(dist1=(da * da).sum(-1), dist2=(db * db).sum(-1), ga=ga, gb=gb, Ka=Ka, Kb=Kb, Sa=Sa, Sb=Sb)


def grad_bound_share(got, ref, K, S):
    """max over the components of |got - ref| / ((K + 6) 2^-24 S), the used share of the derived bound (<= 1 passes; a
    component with S == 0 has to be exactly ref == 0).  Derivation: a term 2 g (t - s) is one rounded difference and one
    rounded product (the doubling is exact), 2 u; a component's K + 1 terms are added once each, a term passing through at
    most K + 3 rounded additions (its lane's chain, then the three additions that join the four lanes); second-order
    parts stay below the 1 u of slack for K <= 5000."""
    err = (got.detach().cpu().double() - ref).abs()
    bound = (K + 6) * U * S
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float('inf')
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


@functools.lru_cache(maxsize=None)
def case(kind, B, N, M):
    """(a, b, restatement (a) of them): computed once and shared; callers do not modify it."""
    a, b = {'random': random_clouds, 'grid': grid_clouds}[kind](B, N, M)
    return a, b, nn_fp32(a, b)
