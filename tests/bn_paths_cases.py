"""The BatchNorm row and pooling kernels (sug_amd/csrc/bn_rows.hip, the pooling half of bnpool.hip; ops.bn_act_rows,
ops.bn_act_pool_cat, ops.bn_update_stats, ops.bn_replay, ops.col_stats, ops.affine_act, ops.bn_coef) on every dispatch path,
for tests/test_bn_paths_host.py and tests/test_gpu_bn_paths.py.  Error measure, bound, margins and the BatchNorm piece are
those of tests/dgcnn_seg_cases.py (err(kernel) <= 8 err(the same formula in fp32 torch) + 1e-7 against fp64);
nothing at module level imports sug_amd.

The layers, per domain group of rows / G rows (pool: B / G clouds) with statistics of their own -- the groups take the running
buffers one after the other, as separate nn.BatchNorm calls would (momentum 0.1, unbiased running variance):
  rows:  out = act(bn(y)),  act = LeakyReLU(slope) (0: ReLU, 1: none)
  pool:  a = act(bn(y)) [B,N,C];  mean over the N rows of a cloud;  max by an EXPLICIT gather at the first n at the maximum of
         the activated value -- the kernels' stated rule (bnpool.hip: the first maximum within a row-lane, the lower row
         across lanes, the lower chunk across chunks) -- so that autograd sends the gradient to exactly that row.  The index
         comes from the fp64 forward; the fp32 run is made to route by it (test_bn_paths_host.py shows its own choice agrees
         wherever the probe is live).

Inputs of a case (seeded by its name): y = randn + a per-channel offset in [-1, 1]; one dominant row per group, DOMINANT x
the row in front of it, never the group's first row: the statistics are taken about the first row of the group (common.h),
and DESIGN 4c records what an outlier there costs -- that limit is kept out of these cases.  So is its milder form (DESIGN
4f): the fp32 partial sums run serially over the rows of a lane and over the row-lanes, and carry n (p - mean) of the
pivot p; with the first row as drawn, 3 sigma off the mean in one of 4095 channels ((p - mean)^2 / var = 9.4), the scalar
kernel's var was off by 5e-6 of itself and dy by 1.2e-6 against 1.3e-7 of fp32 torch.  The first row of each group lies
a quarter of its drawn distance from the channel's offset.  gamma of alternating sign with
|gamma| >= 0.25; beta; running buffers off their defaults; one probe per output.  The rows probe is zeroed where the fp64
pre-activation lies within TAU_KINK * max(1, rms) of 0 (slope 1 has no kink).  The pool's gmax probe is zeroed at a (cloud,
channel) whose top-1 to top-2 gap, exact copies of the winner aside, is below TAU_GAP * rms of the group's activations; and
because the mean sends a gradient through the activation of EVERY row, the pool inputs are drawn again (at most 32 times)
until no pre-activation lies within KINK1 * max(1, rms) of the kink, as dgcnn_seg_cases.block_case does for its first layer.

ROWS_CASES / POOL_CASES / STATS_CASES hold the smallest shapes at which each kernel and regime of the dispatch exists;
ROWS_EXPECT / POOL_EXPECT / STATS_EXPECT state it, test_bn_paths_host.py holds it against the launch arithmetic restated
below and against the library's own answer (ops.bn_rows_plan).  The choice of the pool backward's apply kernel is restated
here only (pool_apply): it is three lines of sug_bn_act_pool_bwd with no query of its own."""
import functools

import torch
import torch.nn.functional as F

from dgcnn_seg_cases import (gen, err, within, act, _bn, FACTOR, FLOOR, TAU_KINK, TAU_GAP, KINK1, MAX_ZEROED, EPS,   # noqa: F401
                             MOMENTUM, DOMINANT)

STATS_BLOCKS = 1024                 # SUG_STATS_BLOCKS (include/sug_amd.h)
STATS_ROWS = STATS_BLOCKS - 8       # SUG_STATS_ROWS (sug_amd/csrc/common.h)
MAX_GROUPS = 16                     # groups of one launch (launch_col_reduce, the pool's grouped entry points)
NS = 4                              # row chunks per cloud (bnpool.hip)


# ----------------------------------------------------------------------------- the launch arithmetic, restated
def col_plan(rows, C, ld=None, groups=1, own_ws=False, mode=0, aligned=True):
    """launch_col_reduce (bn_rows.hip) over `groups` blocks of `rows` rows -> (vec, lanes, rpb, grid); grid -1: refused."""
    ld = C if ld is None else ld
    if C % 4 == 0 and ld % 4 == 0 and aligned:
        lx = 1
        while lx < C // 4 and lx < 256:
            lx *= 2
        ly = 256 // lx
        share = 1 if own_ws else groups
        rpb = max((rows * share + STATS_ROWS - 1) // STATS_ROWS, 4 * ly)
        rpb = (rpb + ly - 1) // ly * ly
        grid = (rows + rpb - 1) // rpb
        return True, lx, rpb, -1 if grid * share > STATS_ROWS or groups > MAX_GROUPS else grid
    cw = 1
    while cw < C and cw < 256:
        cw *= 2
    rpb = max(64 * (256 // cw), 256)
    while (rows + rpb - 1) // rpb > STATS_ROWS:
        rpb *= 2
    return False, cw, rpb, -1 if groups > 1 or mode == 2 else (rows + rpb - 1) // rpb


def trips(C, plan):
    """Channel trips of a lane of the reduce kernel."""
    vec, lanes = plan[0], plan[1]
    return ((C // 4 if vec else C) + lanes - 1) // lanes


def rows_path(rg, C, G, train, ldg=None, galigned=True):
    """What sug_bn_act_rows_fwd / _bwd (layers.cpp) do with G groups of rg rows of a dense, aligned y and a gradient of row
    stride ldg -> (fwd, bwd, the plan of the first column reduction each direction tries)."""
    ldg = C if ldg is None else ldg
    vec = C % 4 == 0
    pf = col_plan(rg, C, C, G, False, 0) if train else None
    if G == 1:
        fwd = ('vec' if vec else 'scalar') if train else 'eval'
    elif not train:
        fwd = 'eval-grouped' if vec else 'eval-loop'               # sug_affine_act_groups, or its refusal: one sug_affine_act per group
    elif pf[3] >= 0:
        fwd = 'grouped'
    else:
        fwd = 'refused-scalar' if not vec else 'refused-groups' if G > MAX_GROUPS else 'refused-grid'
    first = train and ldg % 4 == 0 and vec and galigned
    pb = col_plan(rg, C, ldg, G, False, 2 if first else 1, galigned)
    if first and pb[3] >= 0:
        bwd = 'mode2'                                             # sums without a = scale*G, bn_bwd_apply_vec4_groups_kernel<true>
    elif G > 1 and pb[3] >= 0:
        bwd = 'mode1-grouped' if train else 'eval-grouped'         # eval: dy = a, reduce_partials_fold_kernel
    else:                                                         # one sug_edgeconv_bwd_reduce (+ sug_bn_bwd_apply) per group, sug_fold_groups
        one = col_plan(rg, C, ldg, 1, False, 1, galigned)
        bwd = ('loop-vec' if one[0] else 'loop-scalar') if train else ('eval-loop-vec' if one[0] else 'eval-loop-scalar')
    return fwd, bwd, pf, pb


def pool_apply(C, ld, aligned):
    """The apply kernel of sug_bn_act_pool_bwd (dy is dense and aligned): 'rows' = pool_bwd_apply_rows_kernel."""
    vec = C % 4 == 0 and ld % 4 == 0 and aligned
    if vec and C // 4 <= 256 and 256 % (C // 4) == 0:
        return 'rows'
    return 'vec4' if vec else 'scalar'


def pool_path(B, N, C, G, train, ld=None, aligned=True, grouped=True):
    """ops.bn_act_pool_cat -> (fwd, bwd, apply, the statistics plan): fwd / bwd 'grouped' = every group in each launch
    (sug_bn_act_pool_groups_*), 'loop' = group by group, 'refused' = the backward's B * NS > SUG_STATS_BLOCKS."""
    ld = C if ld is None else ld
    Bg = B // G
    vec = C % 4 == 0 and ld % 4 == 0 and aligned
    try_groups = grouped and train and 1 < G <= MAX_GROUPS
    plan = col_plan(Bg * N, C, ld, G if try_groups else 1, try_groups, 0, aligned) if train else None
    fwd = 'grouped' if try_groups and plan[3] >= 0 and vec else 'loop'
    ap = pool_apply(C, ld, aligned)
    if try_groups and ap == 'rows' and B * NS <= STATS_BLOCKS:
        bwd = 'grouped'
    else:
        bwd = 'loop' if Bg * NS <= STATS_BLOCKS else 'refused'
    return fwd, bwd, ap, plan


# ----------------------------------------------------------------------------- the tables
#  name: (rows, C, G, slope, train, options)       options: shape (the input's shape on the device), gslice ('mis': the
#  gradient is wide[:, 1:1+C], 'pad': wide[:, 4:4+C]), pre (a second call with pre=(out, coef)), scale (of y)
ROWS_CASES = {
    'vec-g1': (300, 64, 1, 0.2, True, {}),
    'vec-g2': (600, 64, 2, 0.01, True, {}),
    'vec-g2-4d': (600, 64, 2, 0.0, True, {'shape': (6, 1, 100, 64)}),
    'g16': (640, 32, 16, 0.0, True, {}),
    'g17': (680, 32, 17, 0.2, True, {}),                           # more than 16 groups: refused both ways
    'grid-overflow': (16 * 506, 512, 16, 0.01, True, {}),          # rpb 8, grid 64: 16 * 64 > 1016 partial rows
    'rpb-g1': (4070, 1024, 1, 1.0, True, {}),                      # rpb 5 > 4 ly
    'rpb-g2': (4080, 1024, 2, 0.2, True, {}),
    'c1028': (300, 1028, 1, 0.0, True, {}),                        # C/4 = 257: a second float4 trip
    'c4096': (64, 4096, 1, 0.01, True, {}),                        # the limit: 4 trips
    'c4095': (64, 4095, 1, 0.2, True, {}),                         # scalar, 16 trips, ONE row-lane: a thread sums all rows of a column
    'c1': (300, 1, 1, 0.2, True, {}),                              # 256 row-lanes: what made col_reduce_kernel fold them in fp64
    'c3': (300, 3, 1, 0.0, True, {}),
    'c7': (300, 7, 1, 1.0, True, {}),
    'c70-g1': (600, 70, 1, 0.01, True, {}),                        # scalar, three workgroups, the last partial
    'c70-g2': (1200, 70, 2, 0.2, True, {}),                        # scalar under groups: refused both ways
    # 2 rows per group, 126 of 128 row-lanes idle.  With two rows xhat = +-sqrt(var / (var + eps)) and dy is eps / (var + eps)
    # of its terms: at unit scale nothing but cancellation is left of it, in fp32 torch as in the kernel.  y is scaled to
    # var ~ eps, where dy is a well-conditioned number again
    'two-rows': (4, 8, 2, 0.2, True, {'scale': 2.0 ** -10}),
    'eval-vec-g1': (300, 64, 1, 0.2, False, {}),
    'eval-vec-g2': (600, 64, 2, 0.0, False, {}),
    'eval-scalar-g2': (1200, 70, 2, 0.01, False, {}),
    'gmis-g1': (300, 64, 1, 0.2, True, {'gslice': 'mis'}),
    'gpad-g1': (300, 64, 1, 0.0, True, {'gslice': 'pad'}),
    'gmis-g2': (600, 64, 2, 0.01, True, {'gslice': 'mis'}),
    'gpad-g2': (600, 64, 2, 0.2, True, {'gslice': 'pad'}),
    'pre': (600, 64, 2, 0.2, True, {'pre': True}),
}
GWIDE = 8                           # the wider gradient tensor has C + GWIDE columns

# fwd / bwd: rows_path's words; plan: (vec, lanes, rpb, grid) of the forward's first column reduction (None in eval mode);
# bplan: of the backward's; trips: channel trips of a lane of the forward reduction
ROWS_EXPECT = {
    'vec-g1': dict(fwd='vec', bwd='mode2', plan=(True, 16, 64, 5), bplan=(True, 16, 64, 5), trips=1),
    'vec-g2': dict(fwd='grouped', bwd='mode2', plan=(True, 16, 64, 5), bplan=(True, 16, 64, 5), trips=1),
    'vec-g2-4d': dict(fwd='grouped', bwd='mode2', plan=(True, 16, 64, 5), bplan=(True, 16, 64, 5), trips=1),
    'g16': dict(fwd='grouped', bwd='mode2', plan=(True, 8, 128, 1), bplan=(True, 8, 128, 1), trips=1),
    'g17': dict(fwd='refused-groups', bwd='loop-vec', plan=(True, 8, 128, -1), bplan=(True, 8, 128, -1), trips=1),
    'grid-overflow': dict(fwd='refused-grid', bwd='loop-vec', plan=(True, 128, 8, -1), bplan=(True, 128, 8, -1), trips=1),
    'rpb-g1': dict(fwd='vec', bwd='mode2', plan=(True, 256, 5, 814), bplan=(True, 256, 5, 814), trips=1),
    'rpb-g2': dict(fwd='grouped', bwd='mode2', plan=(True, 256, 5, 408), bplan=(True, 256, 5, 408), trips=1),
    'c1028': dict(fwd='vec', bwd='mode2', plan=(True, 256, 4, 75), bplan=(True, 256, 4, 75), trips=2),
    'c4096': dict(fwd='vec', bwd='mode2', plan=(True, 256, 4, 16), bplan=(True, 256, 4, 16), trips=4),
    'c4095': dict(fwd='scalar', bwd='loop-scalar', plan=(False, 256, 256, 1), bplan=(False, 256, 256, 1), trips=16),
    'c1': dict(fwd='scalar', bwd='loop-scalar', plan=(False, 1, 16384, 1), bplan=(False, 1, 16384, 1), trips=1),
    'c3': dict(fwd='scalar', bwd='loop-scalar', plan=(False, 4, 4096, 1), bplan=(False, 4, 4096, 1), trips=1),
    'c7': dict(fwd='scalar', bwd='loop-scalar', plan=(False, 8, 2048, 1), bplan=(False, 8, 2048, 1), trips=1),
    'c70-g1': dict(fwd='scalar', bwd='loop-scalar', plan=(False, 128, 256, 3), bplan=(False, 128, 256, 3), trips=1),
    'c70-g2': dict(fwd='refused-scalar', bwd='loop-scalar', plan=(False, 128, 256, -1), bplan=(False, 128, 256, -1), trips=1),
    'two-rows': dict(fwd='grouped', bwd='mode2', plan=(True, 2, 512, 1), bplan=(True, 2, 512, 1), trips=1),
    'eval-vec-g1': dict(fwd='eval', bwd='eval-loop-vec', plan=None, bplan=(True, 16, 64, 5), trips=1),
    'eval-vec-g2': dict(fwd='eval-grouped', bwd='eval-grouped', plan=None, bplan=(True, 16, 64, 5), trips=1),
    'eval-scalar-g2': dict(fwd='eval-loop', bwd='eval-loop-scalar', plan=None, bplan=(False, 128, 256, -1), trips=1),
    'gmis-g1': dict(fwd='vec', bwd='loop-scalar', plan=(True, 16, 64, 5), bplan=(False, 64, 256, 2), trips=1),
    'gpad-g1': dict(fwd='vec', bwd='mode2', plan=(True, 16, 64, 5), bplan=(True, 16, 64, 5), trips=1),
    'gmis-g2': dict(fwd='grouped', bwd='loop-scalar', plan=(True, 16, 64, 5), bplan=(False, 64, 256, -1), trips=1),
    'gpad-g2': dict(fwd='grouped', bwd='mode2', plan=(True, 16, 64, 5), bplan=(True, 16, 64, 5), trips=1),
    'pre': dict(fwd='grouped', bwd='mode2', plan=(True, 16, 64, 5), bplan=(True, 16, 64, 5), trips=1),
}

#  name: (B, N, C, G, slope, train, options)       options: yslice ('pad': y = wide[:, :, 4:4+C] with ld = C + 4, 'mis':
#  wide[:, :, 1:1+C]), gslice (the gradient is a column slice of a wider tensor), tie ('chunk' | 'lane' | 'first': the
#  dominant row of cloud 0 of each group copied exactly at a later n; 'const': channels 0 (gamma > 0) and 1 (gamma < 0) of
#  cloud 0 constant), refused (the backward raises)
POOL_CASES = {
    'c64-g1': (2, 67, 64, 1, 0.2, True, {}),
    'c64-g2': (4, 67, 64, 2, 0.2, True, {}),
    'c24': (4, 67, 24, 2, 0.2, True, {}),                          # C/4 = 6 does not divide 256: pool_bwd_apply_kernel<4>
    'c2048': (2, 8, 2048, 2, 0.01, True, {}),                      # C/4 = 512 > 256
    'c100': (4, 20, 100, 2, 0.2, True, {}),                        # a partial 64-channel block
    'c4': (4, 67, 4, 2, 0.2, True, {}),
    'c70-g1': (2, 67, 70, 1, 0.2, True, {}),                       # scalar kernels
    'c70-g2': (4, 67, 70, 2, 0.01, True, {}),
    'n1': (8, 1, 64, 2, 0.2, True, {}),                            # three of the four row chunks empty
    'n2': (4, 2, 64, 2, 0.2, True, {}),
    'n3': (4, 3, 64, 2, 0.2, True, {}),
    'n5': (4, 5, 64, 2, 0.2, True, {}),
    'n300': (2, 300, 64, 1, 0.2, True, {}),                        # several rows per row-lane, five row blocks of the apply kernel
    'g16': (32, 5, 32, 16, 0.2, True, {}),
    'g17': (34, 5, 32, 17, 0.2, True, {}),
    # B * NS = SUG_STATS_BLOCKS.  At C = 8 (128 row-lanes, a serial fp32 fold of 131 terms with the dominant row among them)
    # var came out 8e-7 of itself off and max 4.3e-7 against 3.0e-8 of fp32 torch; C = 64 folds 20 terms
    'b256': (256, 3, 64, 2, 0.2, True, {}),
    'b257': (257, 3, 64, 1, 0.2, True, {'refused': True}),
    'eval-g1': (2, 67, 64, 1, 0.2, False, {}),
    'eval-g2': (4, 67, 64, 2, 0.01, False, {}),
    'ypad-g2': (4, 67, 64, 2, 0.2, True, {'yslice': 'pad'}),
    'ymis-g2': (4, 67, 64, 2, 0.2, True, {'yslice': 'mis'}),
    'gslice-g2': (4, 67, 64, 2, 0.2, True, {'gslice': True}),
    'tie-chunk': (4, 67, 64, 2, 0.2, True, {'tie': 'chunk'}),
    'tie-lane': (4, 67, 64, 2, 0.2, True, {'tie': 'lane'}),
    'tie-first': (4, 67, 64, 2, 0.2, True, {'tie': 'first'}),
    'tie-const': (4, 67, 64, 2, 0.2, True, {'tie': 'const'}),
}
# rows (n1, n2) of the dominant row and its copy at N = 67 (chunks [0,16) [16,33) [33,50) [50,67), 16 row-lanes a chunk)
TIE_ROWS = {'chunk': (5, 40), 'lane': (17, 20), 'first': (16, 32)}
DOM_ROW = 5                                                     # the dominant row of a group without a tie option

# fwd / bwd / apply: pool_path's words with SUG_BN_POOL_GROUPED as shipped; plan: of the statistics
POOL_EXPECT = {
    'c64-g1': dict(fwd='loop', bwd='loop', apply='rows', plan=(True, 16, 64, 3)),
    'c64-g2': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 3)),
    'c24': dict(fwd='grouped', bwd='loop', apply='vec4', plan=(True, 8, 128, 2)),
    'c2048': dict(fwd='grouped', bwd='loop', apply='vec4', plan=(True, 256, 4, 2)),
    'c100': dict(fwd='grouped', bwd='loop', apply='vec4', plan=(True, 32, 32, 2)),
    'c4': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 1, 1024, 1)),
    'c70-g1': dict(fwd='loop', bwd='loop', apply='scalar', plan=(False, 128, 256, 1)),
    'c70-g2': dict(fwd='loop', bwd='loop', apply='scalar', plan=(False, 128, 256, -1)),
    'n1': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 1)),
    'n2': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 1)),
    'n3': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 1)),
    'n5': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 1)),
    'n300': dict(fwd='loop', bwd='loop', apply='rows', plan=(True, 16, 64, 10)),
    'g16': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 8, 128, 1)),
    'g17': dict(fwd='loop', bwd='loop', apply='rows', plan=(True, 8, 128, 1)),
    'b256': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 6)),
    'b257': dict(fwd='loop', bwd='refused', apply='rows', plan=(True, 16, 64, 13)),
    'eval-g1': dict(fwd='loop', bwd='loop', apply='rows', plan=None),
    'eval-g2': dict(fwd='loop', bwd='loop', apply='rows', plan=None),
    'ypad-g2': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 3)),
    'ymis-g2': dict(fwd='loop', bwd='loop', apply='scalar', plan=(False, 64, 256, -1)),
    'gslice-g2': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 3)),
    'tie-chunk': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 3)),
    'tie-lane': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 3)),
    'tie-first': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 3)),
    'tie-const': dict(fwd='grouped', bwd='grouped', apply='rows', plan=(True, 16, 64, 3)),
}

#  name: (op, rows, C, G, layout)      layout of y (update) resp. of out (affine): 'dense', 'pad' (wide[:, 4:4+C]), 'mis' (1:1+C)
STATS_CASES = {}
for _G in (1, 2, 16, 17):
    for _lay in ('dense', 'pad', 'mis'):
        STATS_CASES['update-g%d-%s' % (_G, _lay)] = ('update', 40 * _G, 32, _G, _lay)
STATS_CASES.update({
    'col-stats-pad': ('col_stats', 300, 64, 1, 'pad'),
    'col-stats-mis': ('col_stats', 300, 64, 1, 'mis'),
    'affine-pad': ('affine', 300, 64, 1, 'pad'),
    'affine-mis': ('affine', 300, 64, 1, 'mis'),
    'coef': ('coef', 300, 70, 1, 'dense'),
    'replay': ('replay', 600, 64, 2, 'dense'),
    'replay-g17': ('replay', 680, 32, 17, 'dense'),
})
SWIDE = 8                           # the wider tensor of a 'pad' / 'mis' layout has C + SWIDE columns


def stats_expect(name):
    """'grouped' (sug_col_stats_bn_own_ws: one launch pair) | 'loop' for an update case, with the plan of the reduction it
    tries first; (vec, ...) of the one reduction of col_stats; None for the ops without a column reduction."""
    op, rows, C, G, lay = STATS_CASES[name]
    ld, al = (C, True) if lay == 'dense' else (C + SWIDE, lay == 'pad')
    if op == 'update':
        own = 1 < G                                               # ops.BN_POOL_GROUPED: sug_col_stats_bn_groups_exact
        plan = col_plan(rows // G, C, ld, G if 1 < G <= MAX_GROUPS else 1, 1 < G <= MAX_GROUPS, 0, al)
        return ('grouped' if own and G <= MAX_GROUPS and plan[3] >= 0 else 'loop'), plan
    if op == 'col_stats':
        return 'single', col_plan(rows, C, ld, 1, False, 0, al)
    return None, None


STATS_EXPECT = {
    'update-g1-dense': ('loop', (True, 8, 128, 1)), 'update-g1-pad': ('loop', (True, 8, 128, 1)),
    'update-g1-mis': ('loop', (False, 32, 512, 1)),
    'update-g2-dense': ('grouped', (True, 8, 128, 1)), 'update-g2-pad': ('grouped', (True, 8, 128, 1)),
    'update-g2-mis': ('loop', (False, 32, 512, -1)),
    'update-g16-dense': ('grouped', (True, 8, 128, 1)), 'update-g16-pad': ('grouped', (True, 8, 128, 1)),
    'update-g16-mis': ('loop', (False, 32, 512, -1)),
    'update-g17-dense': ('loop', (True, 8, 128, 1)), 'update-g17-pad': ('loop', (True, 8, 128, 1)),
    'update-g17-mis': ('loop', (False, 32, 512, 1)),
    'col-stats-pad': ('single', (True, 16, 64, 5)), 'col-stats-mis': ('single', (False, 64, 256, 2)),
    'affine-pad': (None, None), 'affine-mis': (None, None), 'coef': (None, None), 'replay': (None, None),
    'replay-g17': (None, None),
}


def rows_shape(name):
    return dict(zip(('rows', 'C', 'G', 'slope', 'train', 'opt'), ROWS_CASES[name]))


def pool_shape(name):
    return dict(zip(('B', 'N', 'C', 'G', 'slope', 'train', 'opt'), POOL_CASES[name]))


def rows_case_path(name):
    s = rows_shape(name)
    gs = s['opt'].get('gslice')
    return rows_path(s['rows'] // s['G'], s['C'], s['G'], s['train'], s['C'] + GWIDE if gs else None, gs != 'mis')


def pool_case_path(name, grouped=True):
    s = pool_shape(name)
    ys = s['opt'].get('yslice')
    return pool_path(s['B'], s['N'], s['C'], s['G'], s['train'], s['C'] + 4 if ys else None, ys != 'mis', grouped)


# ----------------------------------------------------------------------------- inputs
def _params(C, g):
    gl = torch.randn(C, generator=g).abs().clamp_min(0.25)
    sign = 1.0 - 2.0 * (torch.arange(C) % 2)                      # channel 0 positive, channel 1 negative, ...
    return {'gamma': gl * sign, 'beta': torch.randn(C, generator=g) * 0.2,
            'mean': torch.linspace(-0.1, 0.3, C), 'var': torch.linspace(0.6, 1.4, C)}


def _data(n, C, g, G=1):
    """[n,C] = randn + a per-channel offset; the first row of each of the G groups (the pivot of its sums) a quarter of its
    distance from the offset."""
    off = torch.rand(C, generator=g) * 2 - 1
    y = torch.randn(n, C, generator=g) + off
    first = torch.arange(G) * (n // G)
    y[first] = off + 0.25 * (y[first] - off)
    return y


def _near(t, tau):
    return t.abs() < tau * max(1.0, float(t.pow(2).mean().sqrt()))


@functools.lru_cache(maxsize=None)
def rows_inputs(name):
    """y [rows,C], gamma, beta, mean, var, gout [rows,C]; shared, read-only."""
    s = rows_shape(name)
    rows, C, G = s['rows'], s['C'], s['G']
    g = gen('bn-paths-rows', name)
    y = _data(rows, C, g, G) * s['opt'].get('scale', 1.0)
    rg = rows // G
    dom = min(DOM_ROW, rg - 1)                                    # never the group's first row (the pivot)
    for i in range(G):
        y[i * rg + dom] = DOMINANT * y[i * rg + dom - 1]
    c = dict(s, y=y, gout=torch.randn(rows, C, generator=g), dom=dom, **_params(C, g))
    return c


def rows_forward(c, y, gamma, beta):
    """The rows layer of case c -> dict(out, pre, mean, var (the running buffers after the call))."""
    G = c['G']
    rg = c['rows'] // G
    rm, rv = c['mean'].to(y.dtype), c['var'].to(y.dtype)
    pres = []
    for i in range(G):
        t, rm, rv = _bn(y[i * rg:(i + 1) * rg], gamma, beta, rm, rv, c['train'])
        pres.append(t)
    pre = torch.cat(pres)
    return {'out': act(pre, c['slope']), 'pre': pre, 'mean': rm, 'var': rv}


@functools.lru_cache(maxsize=None)
def rows_probe(name):
    """(gout with the elements at the kink zeroed, the share zeroed), from the fp64 forward."""
    c = rows_inputs(name)
    with torch.no_grad():
        pre = rows_forward(c, c['y'].double(), c['gamma'].double(), c['beta'].double())['pre']
    bad = _near(pre, TAU_KINK) if c['slope'] != 1.0 else torch.zeros_like(pre, dtype=torch.bool)
    return torch.where(bad, torch.zeros_like(c['gout']), c['gout']), float(bad.double().mean())


@functools.lru_cache(maxsize=None)
def rows_reference(name, dtype):
    """The restatement in 'float64' / 'float32' with the gradients of the probe: out, pre, mean, var, dy, dgamma, dbeta."""
    c, dt = rows_inputs(name), getattr(torch, dtype)
    leaves = [t.to(dt).clone().requires_grad_(True) for t in (c['y'], c['gamma'], c['beta'])]
    r = rows_forward(c, *leaves)
    grads = torch.autograd.grad(r['out'], leaves, rows_probe(name)[0].to(dt))
    res = {k: v.detach() for k, v in r.items()}
    res.update(dy=grads[0], dgamma=grads[1], dbeta=grads[2])
    return res


def rows_compared(name):
    return ['out', 'dy', 'dgamma', 'dbeta'] + (['mean', 'var'] if rows_shape(name)['train'] else [])


def _pool_draw(name, attempt):
    s = pool_shape(name)
    B, N, C, G = s['B'], s['N'], s['C'], s['G']
    g = gen('bn-paths-pool', name, attempt)
    y = _data(B * N, C, g, G).view(B, N, C)
    Bg, tie = B // G, s['opt'].get('tie')
    flat = y.view(G, Bg * N, C)                                   # the rows of a group
    if tie in TIE_ROWS:
        n1, n2 = TIE_ROWS[tie]
        flat[:, n1] = DOMINANT * flat[:, n1 - 1]                  # cloud 0 of each group
        flat[:, n2] = flat[:, n1]
    else:
        dom = min(DOM_ROW, Bg * N - 1)
        flat[:, dom] = DOMINANT * flat[:, dom - 1]
    if tie == 'const':
        y.view(G, Bg, N, C)[:, 0, :, :2] = 0.5                    # exact in every sum
    return dict(s, y=y, gout=torch.randn(B, 2 * C, generator=g), attempt=attempt, **_params(C, g))


def pool_forward(c, y, gamma, beta, nstar=None):
    """The pool layer of case c on y [B,N,C] -> dict(out [B,2C] = max | mean, pre, nstar [B,C], gap, bad (the (cloud, channel)
    pairs the margin excludes), mean, var); nstar: route by these rows instead of the restatement's own."""
    B, N, C, G = c['B'], c['N'], c['C'], c['G']
    Bg = B // G
    rm, rv = c['mean'].to(y.dtype), c['var'].to(y.dtype)
    outs, pres, ns, bads = [], [], [], []
    for i in range(G):
        yg = y[i * Bg:(i + 1) * Bg]
        t, rm, rv = _bn(yg.reshape(Bg * N, C), gamma, beta, rm, rv, c['train'])
        a = act(t, c['slope']).view(Bg, N, C)
        with torch.no_grad():
            top = a.max(dim=1, keepdim=True).values
            n = torch.where(a == top, torch.arange(N).view(1, N, 1), N).min(dim=1).values          # the first n at the maximum
            second = a.masked_fill(a == top, -float('inf')).max(dim=1).values                        # exact copies of the winner aside
            bads.append((top.squeeze(1) - second) < TAU_GAP * float(a.double().pow(2).mean().sqrt()))
        route = n if nstar is None else nstar[i * Bg:(i + 1) * Bg]
        outs.append(torch.cat((a.gather(1, route.unsqueeze(1)).squeeze(1), a.mean(dim=1)), dim=1))      # the explicit gather
        pres.append(t.view(Bg, N, C)), ns.append(n)
    return {'out': torch.cat(outs), 'pre': torch.cat(pres), 'nstar': torch.cat(ns), 'bad': torch.cat(bads), 'mean': rm, 'var': rv}


@functools.lru_cache(maxsize=None)
def pool_inputs(name):
    """y [B,N,C], gamma, beta, mean, var, gout [B,2C] with the excluded gmax entries zeroed, zeroed (their share), nstar
    (the fp64 forward's rows); drawn again until no pre-activation lies within KINK1 of the kink.  Shared, read-only."""
    for attempt in range(32):
        c = _pool_draw(name, attempt)
        with torch.no_grad():
            r = pool_forward(c, c['y'].double(), c['gamma'].double(), c['beta'].double())
        if not bool(_near(r['pre'], KINK1).any()):
            break
    else:
        raise AssertionError('could not draw %s off the kink of the activation' % name)
    C = c['C']
    gout = c['gout'].clone()
    gout[:, :C] = torch.where(r['bad'], torch.zeros_like(gout[:, :C]), gout[:, :C])
    c.update(gout=gout, zeroed=float(r['bad'].double().mean()), nstar=r['nstar'])
    return c


@functools.lru_cache(maxsize=None)
def pool_reference(name, dtype):
    """The restatement in 'float64' / 'float32' (routed by the fp64 rows) with the gradients of the probe: out, max, mean_n
    (the two halves of out), pre, nstar (its OWN choice), mean, var, dy, dgamma, dbeta."""
    c, dt = pool_inputs(name), getattr(torch, dtype)
    leaves = [t.to(dt).clone().requires_grad_(True) for t in (c['y'], c['gamma'], c['beta'])]
    r = pool_forward(c, *leaves, nstar=c['nstar'])
    grads = torch.autograd.grad(r['out'], leaves, c['gout'].to(dt))
    res = {k: v.detach() for k, v in r.items()}
    res.update(dy=grads[0], dgamma=grads[1], dbeta=grads[2], max=res['out'][:, :c['C']], mean_n=res['out'][:, c['C']:])
    return res


def pool_compared(name):
    return ['max', 'mean_n', 'dy', 'dgamma', 'dbeta'] + (['mean', 'var'] if pool_shape(name)['train'] else [])


# ----------------------------------------------------------------------------- the composed forms (tie-free cases)
def naive_rows(c, y, gamma, beta):
    """F.batch_norm + F.leaky_relu per group on [rows,C] -> (out, running mean, running var)."""
    G, rg = c['G'], c['rows'] // c['G']
    rm, rv = c['mean'].to(y.dtype).clone(), c['var'].to(y.dtype).clone()
    outs = [F.leaky_relu(F.batch_norm(y[i * rg:(i + 1) * rg], rm, rv, gamma, beta, c['train'], MOMENTUM, EPS), c['slope'])
            for i in range(G)]
    return torch.cat(outs), rm, rv


def naive_pool(c, y, gamma, beta):
    """F.batch_norm + F.leaky_relu + max / mean over N per group on [B,N,C] -> (cat(max, mean) [B,2C], mean, var)."""
    B, N, C, G = c['B'], c['N'], c['C'], c['G']
    Bg = B // G
    rm, rv = c['mean'].to(y.dtype).clone(), c['var'].to(y.dtype).clone()
    outs = []
    for i in range(G):
        a = F.leaky_relu(F.batch_norm(y[i * Bg:(i + 1) * Bg].reshape(Bg * N, C), rm, rv, gamma, beta, c['train'], MOMENTUM, EPS),
                         c['slope']).view(Bg, N, C)
        outs.append(torch.cat((a.max(dim=1)[0], a.mean(dim=1)), dim=1))
    return torch.cat(outs), rm, rv


# ----------------------------------------------------------------------------- the statistics ops
@functools.lru_cache(maxsize=None)
def stats_inputs(name):
    """y [rows,C] (a dominant row per group), gamma, beta, mean, var, slope; shared, read-only."""
    op, rows, C, G, lay = STATS_CASES[name]
    g = gen('bn-paths-stats', name)
    y = _data(rows, C, g, G)
    rg = rows // G
    for i in range(G):
        y[i * rg + DOM_ROW] = DOMINANT * y[i * rg + DOM_ROW - 1]
    return dict(op=op, rows=rows, C=C, G=G, lay=lay, y=y, slope=0.2, **_params(C, g))


def moments(y, G):
    """Per group of rows / G rows of y [rows,C] -> (mean [G,C], biased variance [G,C], unbiased) in y's dtype."""
    yg = y.view(G, -1, y.shape[-1])
    return yg.mean(dim=1), yg.var(dim=1, unbiased=False), yg.var(dim=1, unbiased=True)


def recurrence(rm, rv, mean, unbiased, momentum=MOMENTUM):
    """The running buffers after one train-mode call per row of mean / unbiased [G,C], in order."""
    for m, v in zip(mean, unbiased):
        rm, rv = (1 - momentum) * rm + momentum * m, (1 - momentum) * rv + momentum * v
    return rm, rv


def coef_rows(c, y, dtype):
    """coef [G,5,C] = scale | shift | mean | rstd | unbiased variance of the groups of y, in dtype."""
    m, v, u = moments(y.to(dtype), c['G'])
    rstd = 1.0 / torch.sqrt(v + EPS)
    scale = c['gamma'].to(dtype) * rstd
    return torch.stack((scale, c['beta'].to(dtype) - m * scale, m, rstd, u), dim=1)
