"""Torch-facing wrappers over the C ABI (include/sug_amd.h).

Tensors are plumbing here: device memory + the current HIP stream.  Every op
requires fp32/int32 tensors on a HIP device and raises otherwise -- there is no
CPU path.  Feature tensors are point-major rows [B,N,C].
"""
import contextlib
import ctypes
import math
import os as _os

import torch

from ._lib import lib, check, STATS_BLOCKS, CONSTANTS as _H      # _H: the #defines of include/sug_amd.h

class StepContext:
    """The mutable state a forward / training step of this package scopes -- ONE object instead of a dozen module globals (round 6,
    VERDICT r5 #9).  One process drives one GPU, so one context per process: SUGStep, Net_MDA.forward_pair, the call-graph manager
    and bench.py set fields for the duration of a pass (always restoring the previous value), the ops read them.  The old
    module-level names (`ops.BN_GROUPS`, `ops.START_PROVIDER`, `ops.PROFILE`, ...) remain as properties of the module that forward
    to this object, so existing callers and tests keep working.

      bn_groups          G equal contiguous parts of the batch (Net_MDA.forward_pair: source clouds, then target clouds) that the
                         reference sends through the network in G separate forward calls: BatchNorm statistics and running-buffer
                         updates per part, in order
      start_queue        pre-drawn FPS starts of this forward (Net_MDA.forward_pair draws them in the reference's call order:
                         every farthest_point_sample of the source forward, then those of the target forward), consumed by
                         draw_start
      start_provider     None, or a callable (B, N) -> starts: a graph's start feeder (record / provide), a test's table
      geometry_plan      FPS + ball-query results of several encoder passes over ONE batch computed up front
                         (Pointnet2_g.plan_geometry: both depend on the coordinates and the start draws only, so the semantic
                         and the node pass of a step share their launches): a list of (new_xyz, idx) per sample_and_group call,
                         popped in call order by pointnet2_utils.sample_and_group_idx
      profile            None, or {kernel name: [(event, event, shape)]}: bench.py's per-kernel HIP-event timings (see _timed)
      profile_only       None, or the set of name prefixes that get events
      parallel_branches  independent small-kernel chains on forked streams (opt-in; measured slower)
      fused_heads        fused LayerNorm + activation in the FC heads (SUGStep switches it on for its own forwards)
      w16_cache          step-scoped cache of 16-bit weight copies (Point Transformer, fp16 mode) or None
      bn_record          None, or the list collecting (BatchNorm module, batch-statistics coefficients) of a shared prefix
      pending_counts     None, or the deferred num_batches_tracked increments of this pass

    `scoped(**fields)` is the one way a field is set for the duration of a block; `unscoped()` says that no field which must
    block a graph capture is set.  A new field of that kind is added to `unscoped()` and nowhere else."""
    __slots__ = ('bn_groups', 'start_queue', 'start_provider', 'geometry_plan', 'profile', 'profile_only', 'parallel_branches',
                 'fused_heads', 'w16_cache', 'bn_record', 'pending_counts')

    def __init__(self):
        self.bn_groups = 1
        self.start_queue = self.start_provider = self.geometry_plan = None
        self.profile = self.profile_only = None
        self.parallel_branches = False
        self.fused_heads = False
        self.w16_cache = self.bn_record = self.pending_counts = None

    @contextlib.contextmanager
    def scoped(self, **fields):
        """Set the named fields inside the block; on exit (also by an exception) they hold their values of entry again."""
        old = {k: getattr(self, k) for k in fields}
        for k, v in fields.items():
            setattr(self, k, v)
        try:
            yield self
        finally:
            for k, v in old.items():
                setattr(self, k, v)

    def unscoped(self):
        """True when every field that a captured graph would bake in (or that changes what a forward computes) is at rest."""
        return self.bn_groups == 1 and self.start_queue is None and self.geometry_plan is None and \
            self.start_provider is None and self.profile is None and self.bn_record is None


CTX = StepContext()

SIGMA_LIST = (0.01, 0.1, 1, 10, 100)       # model/mmd.py:23


# Independent branches of a step (the two classifier heads, the two attention layers, the three MMD terms) are chains of
# small kernels -- 5-15 us each, launch-latency bound.  Inside a captured hipGraph they can run side by side: with
# PARALLEL_BRANCHES on (SUGStep switches it on for its own forwards when it replays the step from a graph), run_parallel
# forks the branches onto side streams and joins them; autograd runs each branch's backward on the stream of its
# forward, so the backward branches overlap too.  Launched eagerly from Python the extra event records only cost host
# time, hence off by default.  (Measured on ROCm 7.2 / MI355X: also under graph replay it is a loss -- 5.35 vs 5.26 ms per
# DGCNN step -- a cross-stream edge of a hipGraph costs more than the kernels it overlaps; SUG_PARALLEL_BRANCHES=1 opts in.)
_SIDE_STREAMS = {}


def run_parallel(fns):
    """[f() for f in fns], the calls after the first on side streams forked from / joined to the current stream."""
    if not CTX.parallel_branches or len(fns) < 2 or not torch.cuda.is_available():
        return [f() for f in fns]
    main = torch.cuda.current_stream()
    dev = main.device_index
    sides = []
    for i in range(1, len(fns)):
        st = _SIDE_STREAMS.get((dev, i))
        if st is None:
            st = _SIDE_STREAMS[(dev, i)] = torch.cuda.Stream(device=dev)
        st.wait_stream(main)                  # fork point: before any branch is enqueued
        sides.append(st)
    outs = [fns[0]()]
    for f, st in zip(fns[1:], sides):
        with torch.cuda.stream(st):
            outs.append(f())
    for st in sides:
        main.wait_stream(st)                  # join
    return outs


@contextlib.contextmanager
def capture_guard():
    """Around every hipGraph capture of this package.  torch.cuda.graph no longer runs the garbage collector when a capture
    starts (torch >= 2.9: `torch.compiler.config.force_cudagraph_gc` is off), so a dead Python cycle that owns HIP objects -- an
    earlier trainer's captured graphs, tensors of a destroyed graph's private pool -- could be collected IN THE MIDDLE of a
    capture: hipGraphExecDestroy / hipFree under a global-mode capture aborted the process (seen once in a full test run,
    round 6: 'Fatal Python error: Aborted ... Garbage-collecting' inside a captured forward).  The collector stays OFF for the
    duration of the capture (dead cycles wait for the next automatic collection outside it; a full collection here costs
    ~0.1 s in a large process and a step is captured in up to six pieces), and the module-level tensor cache is dropped
    first (its tensors may live in an older graph's pool and would otherwise be released -- by reference count, collector
    or not -- by the first op of the capture that replaces them)."""
    import gc
    clear_rows_cache()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def bn_groups(g):
    """The batch holds g domain groups (see StepContext.bn_groups) inside the block.  Everything per-cloud / per-row is
    oblivious to that; the BatchNorm ops compute statistics and update the running buffers per part, in order, so the result
    is the one of g separate calls."""
    return CTX.scoped(bn_groups=int(g))


def start_queue(q):
    return CTX.scoped(start_queue=list(q) if q is not None else None)


def draw_start(B, N):
    """FPS start indices [B]: the reference draws torch.randint(0, N, (B,)) from the CPU default generator once per
    farthest_point_sample call.  A start queue or a provider (SUGStep's graph mode) hands out the same draws made up front
    -- the provider as device-resident slices, so a step can be replayed."""
    if CTX.start_queue:                 # draws made up front for this forward (Net_MDA.forward_pair: the reference's order)
        t = CTX.start_queue.pop(0)
        if t.numel() != B:
            raise RuntimeError('FPS start plan does not match the encoder (%d starts for %d clouds)' % (t.numel(), B))
        return t
    if CTX.start_provider is not None:
        return CTX.start_provider(B, N)
    G = CTX.bn_groups
    if G > 1 and B % G == 0:        # one CPU-generator draw per reference forward call
        return torch.cat([torch.randint(0, N, (B // G,), dtype=torch.long) for _ in range(G)])
    return torch.randint(0, N, (B,), dtype=torch.long)


def draw_group_start(B, N):
    """One reference forward's draw (B clouds of one domain group), through the graph's start feeder when one is active."""
    if CTX.start_provider is not None:
        return CTX.start_provider(B, N)
    return torch.randint(0, N, (B,), dtype=torch.long)


def _timed(name, shape, call):
    """call(), between two timing events on the launch stream when bench.py profiles this kernel name (CTX.profile = {};
    CTX.profile_only restricts the names: every event pair costs host time, and an eager step is host-bound)."""
    if CTX.profile is None or (CTX.profile_only is not None and not name.startswith(tuple(CTX.profile_only))):
        return call()
    if torch.cuda.is_current_stream_capturing():        # timing events cannot be captured on ROCm
        return call()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    r = call()
    b.record()
    CTX.profile.setdefault(name, []).append((a, b, shape))
    return r


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    # raw handle of the current stream; torch.cuda.current_stream() builds a Stream object (~10 us)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('sug_amd ops run on a HIP device only (got a %s tensor); '
                               'there is no CPU fallback' % t.device)


def _rows3(t):
    """[B,N,C] fp32 rows with unit channel stride -> (B, N, C, ld); copies if the layout
    is not expressible as a single row stride."""
    assert t.dim() == 3 and t.dtype == torch.float32
    B, N, C = t.shape
    if t.stride(2) != 1 or t.stride(0) != N * t.stride(1) or t.stride(1) < C:
        t = t.contiguous()
    return t, B, N, C, t.stride(1)


def _i32(t):
    return t if t.dtype == torch.int32 else t.to(torch.int32)


# ----------------------------------------------------------------------------- index ops
def knn(x, k):
    """x [B,N,C] rows -> idx [B,N,k] int32 (sug_knn)."""
    _need_gpu(x)
    x, B, N, C, ld = _rows3(x.detach())
    idx = torch.empty(B, N, k, dtype=torch.int32, device=x.device)
    check(_timed('knn_C%d' % C, {'B': B, 'N': N, 'C': C, 'k': k},
                 lambda: lib().sug_knn(_p(x), ld, B, N, C, k, _p(idx), _st())), 'sug_knn')
    return idx


def knn_reverse(idx):
    """idx [B,N,k] int32 -> (rev_off [B,N+1], rev_ent [B,N*k])."""
    _need_gpu(idx)
    idx = _i32(idx).contiguous()
    B, N, k = idx.shape
    off = torch.empty(B, N + 1, dtype=torch.int32, device=idx.device)
    ent = torch.empty(B, N * k, dtype=torch.int32, device=idx.device)
    check(lib().sug_knn_reverse(_p(idx), B, N, k, _p(off), _p(ent), _st()), 'sug_knn_reverse')
    return off, ent


def reverse_lists(idx, n_dest, sorted=True, ent=None):
    """idx [B,E] int32 with destinations in [0, n_dest) (others are skipped) -> (rev_off [B,n_dest+1], rev_ent [B,E]):
    per cloud the valid entries in ascending (destination, entry) order and the exclusive prefix of the counts
    (sug_reverse_lists_build).  rev_ent behind rev_off[b, n_dest] entries is not written: `ent`, when given, is the
    [B,E] int32 buffer to fill."""
    _need_gpu(idx)
    idx = _i32(idx).contiguous()
    B, E = idx.shape
    off = torch.empty(B, n_dest + 1, dtype=torch.int32, device=idx.device)
    if ent is None:
        ent = torch.empty(B, E, dtype=torch.int32, device=idx.device)
    assert ent.shape == (B, E) and ent.dtype == torch.int32 and ent.is_contiguous() and ent.device == idx.device
    check(lib().sug_reverse_lists_build(_p(idx), B, E, n_dest, 1 if sorted else 0, _p(off), _p(ent), _st()),
          'sug_reverse_lists_build')
    return off, ent


def reverse_lists_tiled_supported(B, E, N):
    """Does the tiled reverse-list build take B clouds of E entries into N destinations (N <= SUG_REV_TILED_MAX_DEST,
    E <= SUG_REV_TILED_MAX_ENTRIES)?"""
    return bool(lib().sug_reverse_lists_tiled_supported(B, E, N))


def reverse_lists_tiled(idx, n_dest, tile=0, ent=None):
    """The lists of reverse_lists for clouds of any size within reverse_lists_tiled_supported, by the build that streams
    a cloud's entries through LDS in tiles of `tile` entries (0: the library's choice, else a multiple of 1024 up to
    SUG_REV_TILED_MAX_TILE, taken as given): sug_reverse_lists_tiled.  `ent` as in reverse_lists."""
    _need_gpu(idx)
    idx = _i32(idx).contiguous()
    B, E = idx.shape
    off = torch.empty(B, n_dest + 1, dtype=torch.int32, device=idx.device)
    if ent is None:
        ent = torch.empty(B, E, dtype=torch.int32, device=idx.device)
    assert ent.shape == (B, E) and ent.dtype == torch.int32 and ent.is_contiguous() and ent.device == idx.device
    check(lib().sug_reverse_lists_tiled(_p(idx), B, E, n_dest, tile, _p(off), _p(ent), _st()), 'sug_reverse_lists_tiled')
    return off, ent


def fps(xyz, npoint, start):
    """xyz [B,N,3], start [B] (any int dtype/device) -> [B,npoint] int32."""
    _need_gpu(xyz)
    xyz = xyz.detach().contiguous()
    B, N, _ = xyz.shape
    start = start.to(device=xyz.device, dtype=torch.int32, non_blocking=True)
    out = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
    check(lib().sug_fps(_p(xyz), _p(start), B, N, npoint, _p(out), _st()), 'sug_fps')
    return out


def ball_query(xyz, query, radius, nsample):
    """xyz [B,N,3], query [B,S,3] -> [B,S,nsample] int32; r^2 rounded to fp32 the way torch
    rounds the python scalar in `sqrdists > radius ** 2` (model/point_utils.py:102)."""
    _need_gpu(xyz, query)
    xyz, query = xyz.detach().contiguous(), query.detach().contiguous()
    B, N, _ = xyz.shape
    S = query.shape[1]
    r2 = float(torch.tensor(radius ** 2, dtype=torch.float32))
    out = torch.empty(B, S, nsample, dtype=torch.int32, device=xyz.device)
    check(lib().sug_ball_query(_p(xyz), _p(query), B, N, S, r2, nsample, _p(out), _st()), 'sug_ball_query')
    return out


def knn_query(xyz, query, k, want_dist=False, direct=False):
    """k nearest of xyz [B,N,3] for each query [B,S,3] (sort semantics) -> idx [B,S,k].
    direct: distances as sum((q - p)^2) (Point Transformer path) instead of the expanded form."""
    _need_gpu(xyz, query)
    xyz, query = xyz.detach().contiguous(), query.detach().contiguous()
    B, N, _ = xyz.shape
    S = query.shape[1]
    idx = torch.empty(B, S, k, dtype=torch.int32, device=xyz.device)
    dist = torch.empty(B, S, k, dtype=torch.float32, device=xyz.device) if want_dist else None
    fn = lib().sug_knn_query_direct if direct else lib().sug_knn_query
    check(fn(_p(xyz), _p(query), B, N, S, k, _p(idx), _p(dist), _st()), 'sug_knn_query')
    return (idx, dist) if want_dist else idx


def ball_query_multi(xyz, query, radii, nsamples):
    """ball_query for 1 <= R <= 4 radii in one launch (every distance computed once): xyz [B,N,3], query [B,S,3] ->
    a list of R [B,S,nsample_r] int32 tensors, each equal to ball_query(xyz, query, radius_r, nsample_r) bit for bit."""
    _need_gpu(xyz, query)
    xyz, query = xyz.detach().contiguous(), query.detach().contiguous()
    B, N, _ = xyz.shape
    S = query.shape[1]
    R = len(radii)
    if R != len(nsamples) or not 1 <= R <= 4:
        raise RuntimeError('ball_query_multi: need 1..4 radii and as many list lengths (got %d / %d)' % (R, len(nsamples)))
    outs = [torch.empty(B, S, int(ns), dtype=torch.int32, device=xyz.device) for ns in nsamples]
    r2 = (ctypes.c_float * R)(*[float(torch.tensor(r ** 2, dtype=torch.float32)) for r in radii])
    ns = (ctypes.c_int32 * R)(*[int(n) for n in nsamples])
    check(lib().sug_ball_query_multi(_p(xyz), _p(query), B, N, S, R, r2, ns, _ptrs(outs), _st()), 'sug_ball_query_multi')
    return outs


def three_nn_raw(query, cand, direct=False):
    """direct: distances as sum((q - c)^2) over x, y, z (model/PTran_utils.py:36) instead of the expanded form."""
    _need_gpu(query, cand)
    query, cand = query.detach().contiguous(), cand.detach().contiguous()
    B, N, _ = query.shape
    S = cand.shape[1]
    idx = torch.empty(B, N, 3, dtype=torch.int32, device=query.device)
    dist = torch.empty(B, N, 3, dtype=torch.float32, device=query.device)
    if direct:
        check(lib().sug_three_nn_direct(_p(query), _p(cand), B, N, S, _p(idx), _p(dist), _st()), 'sug_three_nn_direct')
    else:
        check(lib().sug_three_nn(_p(query), _p(cand), B, N, S, _p(idx), _p(dist), _st()), 'sug_three_nn')
    return idx, dist


class _FPInterp(torch.autograd.Function):
    """cat(points1, 3-NN inverse-distance interpolation of src) of PointNetFeaturePropagation.forward
    (model/pointnet2_utils.py:305-312): the interpolation is written into its column slice of the [B,N,D1+D2] row
    buffer (sug_fp_interp_fwd), points1 is copied into the other.  Backward: d src by destination row over the sorted
    reverse lists of idx3 (sug_fp_interp_bwd: no atomics, bit-identical run to run); d points1 is a view of g."""

    @staticmethod
    def forward(ctx, points1, src, idx3, d3):
        _need_gpu(points1, src, idx3, d3)
        src, B, S, D2, lds = _rows3(src)
        N = idx3.shape[1]
        D1 = 0 if points1 is None else points1.shape[2]
        out = torch.empty(B, N, D1 + D2, dtype=torch.float32, device=src.device)
        if D1:
            out[:, :, :D1].copy_(points1)
        w3 = torch.empty(B, N, 3, dtype=torch.float32, device=src.device)
        dst = ctypes.c_void_p(out.data_ptr() + 4 * D1)
        check(lib().sug_fp_interp_fwd(_p(src), lds, _p(idx3), _p(d3), B, N, S, D2, dst, D1 + D2, _p(w3), _st()),
              'sug_fp_interp_fwd')
        ctx.save_for_backward(idx3, w3)
        ctx.meta = (B, N, S, D1, D2)
        return out

    @staticmethod
    def backward(ctx, g):
        idx3, w3 = ctx.saved_tensors
        B, N, S, D1, D2 = ctx.meta
        g = g.contiguous()
        dsrc = None
        if ctx.needs_input_grad[1]:
            dsrc = torch.empty(B, S, D2, dtype=torch.float32, device=g.device)
            off = torch.empty(B, S + 1, dtype=torch.int32, device=g.device)
            ent = torch.empty(B, 3 * N, dtype=torch.int32, device=g.device)
            gs = ctypes.c_void_p(g.data_ptr() + 4 * D1)
            check(lib().sug_fp_interp_bwd(gs, D1 + D2, _p(idx3), _p(w3), B, N, S, D2, _p(off), _p(ent), _p(dsrc), D2, _st()),
                  'sug_fp_interp_bwd')
        return (g[:, :, :D1] if D1 and ctx.needs_input_grad[0] else None), dsrc, None, None


def fp_interp(xyz1, xyz2, points1, points2, direct=False):
    """Rows form of feature propagation's interpolation: xyz1 [B,N,3], xyz2 [B,S,3], points1 [B,N,D1] or None, points2
    [B,S,D2] -> [B,N,D1+D2] = cat(points1, interp).  S == 1 broadcasts points2 (model/pointnet2_utils.py:298-299), S == 2
    is an error as in the reference (its weight.view(B, N, 3, 1) fails on two columns).  The coordinates are data: the
    reference's gradient through the distances is not formed, and asking for it raises."""
    _need_gpu(xyz1, xyz2, points1, points2)
    if xyz1.requires_grad or xyz2.requires_grad:
        raise RuntimeError('fp_interp: no gradient flows to the coordinates (xyz1 / xyz2 require grad); the interpolation '
                           'weights are treated as constants -- pass detached coordinates')
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    if S == 1:
        interp = points2.expand(B, N, points2.shape[2])
        return interp.contiguous() if points1 is None else torch.cat([points1, interp], dim=-1)
    if S == 2:
        raise RuntimeError('feature propagation needs S == 1 or S >= 3 coarse points: with S = 2 the reference itself fails '
                           '(three neighbours are taken of two candidates)')
    idx3, d3 = three_nn_raw(xyz1, xyz2, direct=direct)
    return _FPInterp.apply(points1, points2, idx3, d3)


class _ThreeNN(torch.autograd.Function):
    """dist3 is differentiable w.r.t. the candidate (node) positions:
    d/dc |q-c|^2 = 2(c-q); the query cloud is an input and gets no gradient."""

    @staticmethod
    def forward(ctx, query, cand):
        idx, dist = three_nn_raw(query, cand)
        ctx.save_for_backward(query, cand, idx)
        ctx.mark_non_differentiable(idx)
        return idx, dist

    @staticmethod
    def backward(ctx, _gidx, gdist):
        query, cand, idx = ctx.saved_tensors
        B, N, _ = query.shape
        S = cand.shape[1]
        li = idx.long().view(B, N * 3)
        sel = torch.gather(cand, 1, li.unsqueeze(-1).expand(B, N * 3, 3)).view(B, N, 3, 3)
        g = (2.0 * gdist).unsqueeze(-1) * (sel - query.unsqueeze(2))          # [B,N,3,3]
        gc = torch.zeros(B, S, 3, device=cand.device, dtype=cand.dtype)
        gc.scatter_add_(1, li.unsqueeze(-1).expand(B, N * 3, 3), g.view(B, N * 3, 3))
        return None, gc


def three_nn(query, cand):
    """-> (idx3 [B,N,3] int32, dist3 [B,N,3]); dist3 carries gradient to `cand`."""
    return _ThreeNN.apply(query, cand)


# ----------------------------------------------------------------------------- gathers
SCATTER_ORDERED = _os.environ.get('SUG_SCATTER_ORDERED', '1') != '0'      # index_points backward in a fixed order (0: float atomics)


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, idx):
        _need_gpu(feat, idx)
        feat_c, B, N, C, ld = _rows3(feat)
        idx2 = _i32(idx).reshape(B, -1).contiguous()
        S = idx2.shape[1]
        out = torch.empty(B, S, C, dtype=torch.float32, device=feat.device)
        check(lib().sug_gather_rows(_p(feat_c), ld, _p(idx2), B, N, S, C, _p(out), C, _st()), 'sug_gather_rows')
        ctx.save_for_backward(idx2)
        ctx.shape = (B, N, C)
        return out.view(*idx.shape, C)

    @staticmethod
    def backward(ctx, g):
        (idx2,) = ctx.saved_tensors
        B, N, C = ctx.shape
        S = idx2.shape[1]
        g = g.reshape(B, S, C).contiguous()
        L = lib()
        if SCATTER_ORDERED and L.sug_scatter_rows_ordered_supported(B, N, S):
            # fixed summation order (sorted reverse lists): index_points' backward reproducible bit for bit
            d = torch.empty(B, N, C, dtype=torch.float32, device=g.device)
            ws = torch.empty(L.sug_scatter_rows_workspace(B, N, S), dtype=torch.int32, device=g.device)
            check(L.sug_scatter_rows_ordered(_p(g), C, _p(idx2), B, N, S, C, _p(d), C, _p(ws), _st()), 'sug_scatter_rows_ordered')
            return d, None
        d = torch.zeros(B, N, C, dtype=torch.float32, device=g.device)
        check(L.sug_scatter_add_rows(_p(g), C, _p(idx2), B, N, S, C, _p(d), C, _st()), 'sug_scatter_add_rows')
        return d, None


def reverse_lists_fit(B, N, E):
    """Do E index entries per cloud into N destinations fit the LDS-resident reverse-list build (what the ordered
    backwards of gather_rows and of the first set-abstraction layer on neighbour lists need)?"""
    return bool(lib().sug_scatter_rows_ordered_supported(B, N, E))


def gather_rows(feat, idx):
    """feat [B,N,C], idx [B,S] or [B,S,K] -> [B,S(,K),C]  (index_points)."""
    return _GatherRows.apply(feat, idx)


class _GroupMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, idx, pre=None):
        _need_gpu(feat, idx)
        if pre is not None:                     # (out, arg) of this pass from sa_glue_passes: no launch here
            out, arg = pre
            B, N, C = feat.shape
        else:
            feat_c, B, N, C, ld = _rows3(feat)
            idx = _i32(idx).contiguous()
            out, arg = _group_max_raw(feat_c, ld, B, idx, N, C)
        ctx.save_for_backward(arg)
        ctx.shape = (B, N, C)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        B, N, C = ctx.shape
        S = arg.shape[1]
        g = g.contiguous()
        d = torch.zeros(B, N, C, dtype=torch.float32, device=g.device)
        check(lib().sug_group_max_bwd(_p(g), _p(arg), B, N, S, C, _p(d), C, _st()), 'sug_group_max_bwd')
        return d, None, None


def _group_max_raw(feat_c, ld, Bsrc, idx, N, C):
    """(out, arg) [B,S,C] of idx [B,S,ns] over B = P * Bsrc pass-major clouds that read feat_c [Bsrc,N,ld]."""
    B, S, ns = idx.shape
    out = torch.empty(B, S, C, dtype=torch.float32, device=feat_c.device)
    arg = torch.empty(B, S, C, dtype=torch.int32, device=feat_c.device)
    if Bsrc == B:
        check(lib().sug_group_max(_p(feat_c), ld, _p(idx), B, N, S, ns, C, _p(out), _p(arg), _st()), 'sug_group_max')
    else:
        check(lib().sug_group_max_shared(_p(feat_c), ld, Bsrc, _p(idx), B, N, S, ns, C, _p(out), _p(arg), _st()),
              'sug_group_max_shared')
    return out, arg


def group_max(feat, idx, pre=None):
    """max_j feat[b, idx[b,s,j], :] -> [B,S,C].  pre: this pass's (out, arg) where sa_glue_passes has computed them."""
    return _GroupMax.apply(feat, idx, pre)


# ----------------------------------------------------------------------------- per-point linear
# (rows, M, N) of weight gradients for which the TUNED library GEMM beats sug_linear_dw (filled by
# sug_amd.tuning.enable_tuned_gemms from a measured table; empty = always the library's own kernel).
DW_LIBRARY_SHAPES = set()
DW_FORCE_LIBRARY = False        # tuning runs: every weight gradient through the library
DW_SHAPE_LOG = None             # tuning runs: list collecting the (rows, M, N) seen
# measured on MI355X (graph mode, C2 step): the library's selection is 0.1-0.2 ms per step faster for these
# forward GEMMs, tuned table or not -- the own kernel stays opt-in (SUG_OWN_ROWS_GEMM=1)
OWN_ROWS_GEMM = _os.environ.get('SUG_OWN_ROWS_GEMM', '0') == '1'            # forward y = x.W^T of skinny layers (K in {64,128}, Co % 128 == 0) by sug_rows_gemm


class _LinearRows(torch.autograd.Function):
    """y = x . W^T (+ b) over rows; the weight gradient g^T . x (K = rows = B*N, small output)
    runs in sug_linear_dw instead of a rocBLAS GEMM that does not split K."""

    @staticmethod
    def forward(ctx, x, weight, bias, pre=None):
        M, N = weight.shape
        x2 = x.reshape(-1, N)
        if pre is not None:
            # the values an earlier pass computed from the same x and weights (a shared encoder prefix): no launch, a fresh
            # alias of them as this node's output; the backward is this node's own
            y = pre.detach()
        elif OWN_ROWS_GEMM and N in (64, 128) and M % 128 == 0 and x2.shape[0] >= 4096 and x2.stride(1) == 1 \
                and x2.stride(0) % 4 == 0 and x2.data_ptr() % 16 == 0 and weight.is_contiguous():
            # fp32 MFMA kernel of the library (the rocBLAS selection for these skinny shapes is 2-3x slower)
            y = torch.empty(x2.shape[0], M, dtype=torch.float32, device=x.device)
            check(_timed('rows_gemm_K%d_Co%d' % (N, M), {'B': x2.shape[0], 'N': 1, 'k': N, 'Co': M},
                         lambda: lib().sug_rows_gemm(_p(x2), x2.stride(0), x2.shape[0], N, _p(weight.detach()),
                                                     _p(None if bias is None else bias.detach()), M, _p(y), M, _st())),
                  'sug_rows_gemm')
            y = y.view(*x.shape[:-1], M)
        else:
            y = torch.nn.functional.linear(x, weight, bias)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        M, N = weight.shape
        dx, dw, db = linear_rows_backward(x.reshape(-1, N), weight, g.reshape(-1, M), ctx.needs_input_grad[0],
                                          ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        return (None if dx is None else dx.view(x.shape)), dw, db, None


DW_BMM = _os.environ.get('SUG_DW_BMM', '1') == '1'


def _dw_bmm_chunks(R, M, N, g2, x2):
    """Row chunks for the batched-GEMM form of a weight gradient (0 = use sug_linear_dw): outputs >= 128 x 128 (or
    256 x 64), dense operands, chunks of ~4096 rows (8 .. 64 chunks)."""
    if not DW_BMM or M * N < 128 * 128 or min(M, N) < 64 or g2.stride(0) != M or x2.stride(0) != N or \
            g2.stride(1) != 1 or x2.stride(1) != 1:
        return 0
    S = 64
    while S > 8 and R // S < 4096:
        S //= 2
    return S if (R % S == 0 and R // S >= 1024) else 0


def linear_rows_backward(x2, weight, g2, need_dx, need_dw, need_db):
    """Gradients of y = x2 . weight^T (+ b) for rows x2 [R, N], g2 [R, M]: dx by the library GEMM, the weight gradient
    g^T . x (K = rows, small output) by sug_linear_dw(_bias) -- with the bias gradient from the same pass over g."""
    M, N = weight.shape
    if g2.stride(1) != 1:
        g2 = g2.contiguous()
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    R = g2.shape[0]
    dx = dw = db = None
    if need_dx:
        dx = g2 @ weight
    if need_dw:
        if DW_SHAPE_LOG is not None:
            DW_SHAPE_LOG.append((R, M, N))
        # (not while a step graph is being captured: the library's split-K solutions for these K = rows shapes
        # clear their output with a memset, and memset nodes of a replayed hipGraph were not reliably ordered in
        # front of the accumulating kernels on ROCm 7 -- see sug_mmd_rbf_value -- which showed as NaN weights
        # after tens to hundreds of replays)
        lib_ok = DW_FORCE_LIBRARY or ((R, M, N) in DW_LIBRARY_SHAPES and not torch.cuda.is_current_stream_capturing())
        S = _dw_bmm_chunks(R, M, N, g2, x2) if not need_db else 0
        if M * N > 512 * 512 or lib_ok:
            dw = g2.t() @ x2            # larger than any encoder layer, or the tuned library GEMM is faster
        elif S:
            # outputs of 128 x 128 and more: the library's GEMM kernels beat the one-wave MFMA tiles of sug_linear_dw
            # (512 x 512 at 65536 rows: 240 vs 335 us) once K = rows is split by BATCHING over row chunks -- no split-K
            # solution, hence no memset node -- and the partials are folded by sug_linear_dw's ordered reduce
            # (outside TunableOp: its look-up of a shape that is not in the recorded table ends in a hipBLASLt call that
            # is not permitted while a stream is capturing; the default heuristic's batched kernel is)
            import torch.cuda.tunable as _tn
            tuned = _tn.is_enabled()
            if tuned:
                _tn.enable(False)
            try:
                part = torch.bmm(g2.view(S, R // S, M).transpose(1, 2), x2.view(S, R // S, N))
            finally:
                if tuned:
                    _tn.enable(True)
            dw = torch.empty(M, N, dtype=torch.float32, device=g2.device)
            check(lib().sug_linear_dw_fold(_p(part), S, M * N, _p(dw), _st()), 'sug_linear_dw_fold')
        else:
            dw = torch.empty(M, N, dtype=torch.float32, device=g2.device)
            ws = torch.empty(int(lib().sug_linear_dw_workspace(R, M, N)), dtype=torch.float32, device=g2.device)
            if need_db:       # bias gradient from the same pass over g
                db = torch.empty(M, dtype=torch.float32, device=g2.device)
            check(lib().sug_linear_dw_bias(_p(g2), g2.stride(0), _p(x2), x2.stride(0), R, M, N, _p(dw), _p(db), _p(ws),
                                           _st()), 'sug_linear_dw_bias')
    if need_db and db is None:
        db = colsum(g2)
    return dx, dw, db


def linear_rows(x, weight, bias=None, pre=None):
    """F.linear for [..., Cin] rows with many rows and small Cin/Cout (the encoders' 1x1 convs).
    pre: the result an earlier pass of the step computed from the same x and weights; the forward GEMM is then not run."""
    _need_gpu(x, weight)
    if x.dtype != torch.float32:
        raise RuntimeError('sug_amd.ops.linear_rows: fp32 rows only (got %s)' % x.dtype)
    return _LinearRows.apply(x, weight, bias, pre)


# ----------------------------------------------------------------------------- SA-node glue
class _NodeOffset(torch.autograd.Function):
    """(node_off, node_loc) of adapt_layer_off from the projected features (sug_node_offset_*)."""

    @staticmethod
    def forward(ctx, proj, loc, fidx, gidx, pre=None):
        _need_gpu(proj, loc, fidx, gidx)
        proj, loc = proj.contiguous(), loc.detach().contiguous()
        fidx, gidx = _i32(fidx).contiguous(), _i32(gidx).contiguous()
        if pre is not None:                     # (off, nloc) of this pass from sa_glue_passes: no launch here
            off, nloc = pre
        else:
            off, nloc = _node_offset_raw(proj, loc, fidx, gidx)
        ctx.save_for_backward(proj, loc, fidx, gidx)
        ctx.set_materialize_grads(False)
        return off, nloc

    @staticmethod
    def backward(ctx, goff, gnloc):
        proj, loc, fidx, gidx = ctx.saved_tensors
        B, N, _ = proj.shape
        S, ns = gidx.shape[1], gidx.shape[2]
        if goff is None and gnloc is None:
            return None, None, None, None, None
        # nloc = loc[f] + off; an output that took no part in the loss arrives as None (no zero fill + add for it)
        g = (goff if gnloc is None else gnloc if goff is None else goff + gnloc).contiguous()
        dproj = torch.empty_like(proj)              # written (or zeroed) entirely by the entry point
        check(lib().sug_node_offset_bwd(_p(proj), _p(loc), _p(fidx), _p(gidx), _p(g), B, N, S, ns, _p(dproj), _st()),
              'sug_node_offset_bwd')
        return dproj, None, None, None, None


def _node_offset_raw(proj, loc, fidx, gidx):
    """(off, nloc) [B,S,3] over the B = P * Bsrc pass-major clouds of loc / fidx / gidx; proj [Bsrc,N,3] is shared by the passes."""
    Bsrc, N, _ = proj.shape
    B, S, ns = gidx.shape
    off = torch.empty(B, S, 3, dtype=torch.float32, device=proj.device)
    nloc = torch.empty(B, S, 3, dtype=torch.float32, device=proj.device)
    if Bsrc == B:
        check(lib().sug_node_offset_fwd(_p(proj), _p(loc), _p(fidx), _p(gidx), B, N, S, ns, _p(off), _p(nloc), _st()),
              'sug_node_offset_fwd')
    else:
        check(lib().sug_node_offset_fwd_shared(_p(proj), Bsrc, _p(loc), _p(fidx), _p(gidx), B, N, S, ns, _p(off), _p(nloc),
                                               _st()), 'sug_node_offset_fwd_shared')
    return off, nloc


def node_offset(proj, loc, fidx, gidx, pre=None):
    """proj [B,N,3], loc [B,N,3], fidx [B,S], gidx [B,S,ns] -> (node_off [B,S,3], node_loc [B,S,3]).
    pre: this pass's (node_off, node_loc) where sa_glue_passes has computed them."""
    return _NodeOffset.apply(proj, loc, fidx, gidx, pre)


class _Interp3Cat(torch.autograd.Function):
    """cat(fea, inverse-distance 3-NN interpolation of the node features) in one kernel; the
    backward also carries the distance gradient back to the node positions."""

    @staticmethod
    def forward(ctx, fea, node, xyz, nloc, pre=None):
        _need_gpu(fea, node, xyz, nloc)
        fea, B, N, C1, ldf = _rows3(fea)
        node = node.contiguous()
        xyz, nlocd = xyz.detach().contiguous(), nloc.detach().contiguous()
        S, C2 = node.shape[1], node.shape[2]
        if pre is not None:                     # (out, idx3, d3) of this pass from sa_glue_passes: no launch here
            out, idx3, d3 = pre
        else:
            idx3, d3 = three_nn_raw(xyz, nlocd)
            out = _interp3_cat_raw(fea, ldf, C1, B, node, idx3, d3, N)
        ctx.save_for_backward(node, idx3, d3, xyz, nlocd)
        ctx.meta = (B, N, S, C1, C2)
        return out

    @staticmethod
    def backward(ctx, g):
        node, idx3, d3, xyz, nloc = ctx.saved_tensors
        B, N, S, C1, C2 = ctx.meta
        g = g.contiguous()
        L = lib()
        if L.sug_interp3_cat_bwd_lists_supported(B, N, S):
            # fixed summation order (sorted reverse lists of idx3): reproducible bit for bit
            dnode = torch.empty_like(node)
            dnloc = torch.empty_like(nloc)
            off = torch.empty(B, S + 1, dtype=torch.int32, device=g.device)
            ent = torch.empty(B, 3 * N, dtype=torch.int32, device=g.device)
            ddw = torch.empty(B, N, 6, dtype=torch.float32, device=g.device)
            check(L.sug_interp3_cat_bwd_lists(_p(g), C1 + C2, C1, _p(node), _p(idx3), _p(d3), _p(xyz), _p(nloc), B, N, S,
                                              C2, _p(off), _p(ent), _p(ddw), _p(dnode), _p(dnloc), _st()),
                  'sug_interp3_cat_bwd_lists')
        else:
            # 3N entries per cloud do not fit the LDS-resident reverse-list build: the LDS-accumulating form (float
            # atomics into zero-filled gradients; raises when its own [S, C2 + 3] accumulator does not fit either)
            dnode = torch.zeros_like(node)
            dnloc = torch.zeros_like(nloc)
            check(L.sug_interp3_cat_bwd(_p(g), C1 + C2, C1, _p(node), _p(idx3), _p(d3), _p(xyz), _p(nloc), B, N, S, C2,
                                        _p(dnode), _p(dnloc), _st()), 'sug_interp3_cat_bwd')
        return g[:, :, :C1], dnode, None, dnloc, None


def _interp3_cat_raw(fea, ldf, C1, Bsrc, node, idx3, d3, N):
    """out [B,N,C1+C2] over the B = P * Bsrc pass-major clouds of node / idx3 / d3; fea [Bsrc,N,ldf] is shared by the passes."""
    B, S, C2 = node.shape
    out = torch.empty(B, N, C1 + C2, dtype=torch.float32, device=node.device)
    fp, ld = (_p(fea), ldf) if C1 else (None, 0)
    if Bsrc == B:
        check(lib().sug_interp3_cat_fwd(fp, ld, C1, _p(node), _p(idx3), _p(d3), B, N, S, C2, _p(out), C1 + C2, _st()),
              'sug_interp3_cat_fwd')
    else:
        check(lib().sug_interp3_cat_fwd_shared(fp, ld, C1, Bsrc, _p(node), _p(idx3), _p(d3), B, N, S, C2, _p(out), C1 + C2,
                                               _st()), 'sug_interp3_cat_fwd_shared')
    return out


def interp3_cat(fea, node, xyz, nloc, pre=None):
    """fea [B,N,C1], node [B,S,C2], xyz [B,N,3], nloc [B,S,3] -> [B,N,C1+C2].
    pre: this pass's (out, idx3, d3) where sa_glue_passes has computed them."""
    return _Interp3Cat.apply(fea, node, xyz, nloc, pre)


def sa_glue_passes(proj, res, fea, locp, fidx, gidx, k):
    """The SA-node glue of the P passes of a step over ONE batch in one launch per stage (no autograd: the values only).
    proj [B,N,3], res [B,N,C], fea [B,N,C1] are the passes' common operands and are read in place (cloud % B); locp [P*B,N,3],
    fidx [P*B,S], gidx [P*B,S,ns] are pass-major.  Every virtual cloud's result is bit-identical to the per-pass calls
    node_offset -> knn_query -> group_max -> three_nn -> interp3_cat; -> one dict of [P*B,...] tensors, which the passes
    hand to those ops slice by slice as `pre`."""
    _need_gpu(proj, res, fea, locp, fidx, gidx)
    with torch.no_grad():
        B, N, _ = proj.shape
        proj_c, locp = proj.detach().contiguous(), locp.detach().contiguous()
        fidx, gidx = _i32(fidx).contiguous(), _i32(gidx).contiguous()
        if locp.shape[0] % B or fidx.shape[0] != locp.shape[0] or gidx.shape[0] != locp.shape[0] or fea.shape[0] != B or \
                res.shape[0] != B:
            raise RuntimeError('sa_glue_passes: %d planned clouds are not whole passes over a batch of %d' % (locp.shape[0], B))
        off, nloc = _node_offset_raw(proj_c, locp, fidx, gidx)
        gidx2 = knn_query(locp, nloc, k)
        res_c, _, _, C, ldr = _rows3(res.detach())
        node, arg = _group_max_raw(res_c, ldr, B, gidx2, N, C)
        idx3, d3 = three_nn_raw(locp, nloc)
        fea_c, _, _, C1, ldf = _rows3(fea.detach())
        out = _interp3_cat_raw(fea_c, ldf, C1, B, node, idx3, d3, N)
    return {'off': off, 'nloc': nloc, 'gidx2': gidx2, 'node': node, 'arg': arg, 'idx3': idx3, 'd3': d3, 'out': out}


# ----------------------------------------------------------------------------- BN helpers
def bn_coef(stats, gamma, beta, count, eps, momentum, running_mean, running_var, out=None):
    C = gamma.numel()
    coef = torch.empty(5, C, dtype=torch.float32, device=gamma.device) if out is None else out
    check(lib().sug_bn_finalize(_p(stats), _p(gamma), _p(beta), C, float(count), eps, momentum,
                                _p(running_mean), _p(running_var), _p(coef), _st()), 'sug_bn_finalize')
    return coef


def eval_coef(gamma, beta, running_mean, running_var, eps):
    rstd = torch.rsqrt(running_var + eps)
    scale = gamma * rstd
    return torch.stack([scale, beta - running_mean * scale, running_mean, rstd, running_var]).contiguous()


class _BNState:
    """What a fused BatchNorm op needs of its nn.BatchNorm module besides weight and bias (those stay arguments of the
    autograd.Function: autograd must see them): built once at the public entry point, passed to .apply as ONE non-tensor.
    `train` is the kernels' int flag, G = CTX.bn_groups at the time of the call."""
    __slots__ = ('mean', 'var', 'training', 'train', 'eps', 'momentum', 'G')

    def __init__(self, running_mean, running_var, training, eps, momentum):
        self.mean, self.var = running_mean, running_var
        self.training = bool(training)
        self.train = 1 if training else 0
        self.eps, self.momentum, self.G = eps, momentum, CTX.bn_groups


def _bn_state(bn):
    return _BNState(bn.running_mean, bn.running_var, bn.training, bn.eps, bn.momentum)


def _bn_params(gamma, beta, st, C):
    """-> contiguous (gamma, beta) and the [G, 5, C] coefficient buffer of a fused BatchNorm op: left for the kernel to fill
    in train mode, the running-statistics coefficients broadcast over the groups (one copy launch) in eval mode."""
    g, b = gamma.detach().contiguous(), beta.detach().contiguous()
    coef = torch.empty(st.G, 5, C, dtype=torch.float32, device=g.device)
    if not st.training:
        coef.copy_(eval_coef(g, b, st.mean, st.var, st.eps))
    return g, b, coef


def _stats_ws(C, dev):
    """Workspace of the column-statistics reductions over C channels."""
    return torch.empty(STATS_BLOCKS * 2 * C, dtype=torch.float32, device=dev)


def _check_groups(op, n, what, G, seg=None):
    if seg is None and n % G:
        raise RuntimeError('%s: %d %s do not split into %d domain groups' % (op, n, what, G))
    if seg is not None and n % (G * seg):
        raise RuntimeError('%s: %d %s do not split into %d groups of %d-row segments' % (op, n, what, G, seg))


def _dgamma_dbeta(rf):
    """rf [2C] = dbeta | dgamma as the backward kernels write them -> (dgamma, dbeta)."""
    C = rf.numel() // 2
    return rf[C:], rf[:C]


def affine_act(z, coef, slope, out=None):
    """out[...,c] = leaky(scale[c]*z + shift[c]); z [..., C] rows."""
    _need_gpu(z)
    C = z.shape[-1]
    z2 = z.reshape(-1, C)
    if z2.stride(1) != 1:
        z2 = z2.contiguous()
    rows = z2.shape[0]
    if out is None:
        out = torch.empty(rows, C, dtype=torch.float32, device=z.device)
    o2 = out.view(-1, C) if out.is_contiguous() else out
    check(lib().sug_affine_act(_p(z2), z2.stride(0), _p(coef), rows, C, float(slope), _p(o2), o2.stride(0), _st()),
          'sug_affine_act')
    return out.view(*z.shape)


def col_stats(y2, ws=None):
    """y2 [rows, C] (row stride ld) -> fp64 [2C] = column sums, column sums of squares."""
    rows, C = y2.shape
    stats = torch.empty(2 * C, dtype=torch.float64, device=y2.device)
    if ws is None:
        ws = _stats_ws(C, y2.device)
    check(lib().sug_col_stats(_p(y2), y2.stride(0), rows, C, _p(stats), _p(ws), _st()), 'sug_col_stats')
    return stats


def bn_rows_plan(rows, C, ld=None, groups=1, own_ws=False, mode=0, aligned=True):
    """(vec, lanes, rpb, grid) of the column reduction over `groups` blocks of `rows` rows each (sug_bn_rows_plan: the
    function the launch itself is computed from; host-side, no launch).  mode 0: statistics, 1 / 2: the backward sums with /
    without the [rows, C] intermediate; grid -1: the grouped launch is refused and the caller goes group by group."""
    plan = (ctypes.c_int32 * 4)()
    check(lib().sug_bn_rows_plan(rows, C, C if ld is None else ld, groups, int(bool(own_ws)), mode, int(bool(aligned)), plan),
          'sug_bn_rows_plan')
    return bool(plan[0]), plan[1], plan[2], plan[3]


class _BNActRows(torch.autograd.Function):
    """act(BatchNorm(y)) over the rows of y [rows, C]; act = LeakyReLU(slope) (0: ReLU, 1: none).
    Train mode uses batch statistics and updates the running ones like nn.BatchNorm."""

    @staticmethod
    def forward(ctx, y, gamma, beta, st, slope, pre=None):
        _need_gpu(y, gamma)
        C = y.shape[-1]
        y2 = y.reshape(-1, C)
        if y2.stride(1) != 1 or y2.stride(0) != C:
            y2 = y2.contiguous()
        rows = y2.shape[0]
        _check_groups('bn_act_rows', rows, 'rows', st.G)
        dev = y.device
        if pre is not None:
            # (out, coef) an earlier pass computed from the same y and parameters: no launch and no running-statistics
            # update here (the caller replays that); the backward is this node's own
            out, coef = pre[0].detach().reshape(rows, C), pre[1].detach()
        else:
            g, b, coef = _bn_params(gamma, beta, st, C)
            out = torch.empty(rows, C, dtype=torch.float32, device=dev)
            stats = torch.empty(2 * C, dtype=torch.float64, device=dev)
            ws = _stats_ws(C, dev)
            check(lib().sug_bn_act_rows_fwd(_p(y2), C, rows, C, st.G, _p(g), _p(b), st.train, st.eps, st.momentum,
                                            float(slope), _p(st.mean), _p(st.var), _p(coef), _p(out), C,
                                            _p(stats), _p(ws), _st()), 'sug_bn_act_rows_fwd')
        if any(ctx.needs_input_grad[i] for i in (0, 1, 2)):             # y, gamma, beta
            ctx.save_for_backward(y2, coef)
            ctx.meta = (rows, C, float(slope), st.training, tuple(y.shape), st.G)
        ctx.mark_non_differentiable(coef)
        ctx.set_materialize_grads(False)
        return out.view(y.shape), coef

    @staticmethod
    def backward(ctx, gout, _gcoef):
        y2, coef = ctx.saved_tensors
        rows, C, slope, training, shape, G = ctx.meta
        if gout is None:                    # an undefined gradient counts as zeros, as if autograd had materialised it
            gout = torch.zeros_like(y2)
        dy, dgamma, dbeta = _bn_act_rows_backward(gout, y2, coef, rows, C, slope, training, G)
        return dy.view(shape), dgamma, dbeta, None, None, None


def _bn_act_rows_backward(gout, y2, coef, rows, C, slope, training, G):
    """Gradient of act(BatchNorm(y)) over rows (exact train-mode statistics terms): -> (dy [rows, C], dgamma, dbeta)."""
    dev = gout.device
    g2 = gout.reshape(rows, C)
    if g2.stride(1) != 1:
        g2 = g2.contiguous()
    a = torch.empty(rows, C, dtype=torch.float32, device=dev)
    red = torch.empty(G, 2 * C, dtype=torch.float64, device=dev)
    ws = _stats_ws(C, dev)
    dy = torch.empty(rows, C, dtype=torch.float32, device=dev) if training else a
    rf = torch.empty(2 * C, dtype=torch.float32, device=dev)
    check(lib().sug_bn_act_rows_bwd(_p(g2), g2.stride(0), _p(y2), C, _p(coef), rows, C, G, int(training),
                                    slope, _p(a), _p(red), _p(dy), _p(ws), _p(rf), _st()), 'sug_bn_act_rows_bwd')
    return (dy,) + _dgamma_dbeta(rf)


class _SAFirstLayer(torch.autograd.Function):
    """relu(BN(P[idx] - Q)) over the ball-query lists: the first layer of a set-abstraction MLP without the
    grouped [B,S,ns,3+D] tensor (sug_sa_first_fwd / bwd)."""

    @staticmethod
    def forward(ctx, P, Q, idx, gamma, beta, st):
        _need_gpu(P, Q, idx)
        P, Q = P.contiguous(), Q.contiguous()
        idx = _i32(idx).contiguous()
        B, N, C = P.shape
        S, ns = idx.shape[1], idx.shape[2]
        _check_groups('sa_first_layer', B, 'clouds', st.G)
        dev = P.device
        g, b, coef = _bn_params(gamma, beta, st, C)
        Z = torch.empty(B, S, ns, C, dtype=torch.float32, device=dev)
        ws = _stats_ws(C, dev)
        check(lib().sug_sa_first_fwd(_p(P.detach()), C, _p(Q.detach()), _p(idx), B, N, S, ns, C, st.G, _p(g), _p(b),
                                     st.train, st.eps, st.momentum, _p(st.mean), _p(st.var), _p(coef),
                                     _p(Z), _p(ws), _st()), 'sug_sa_first_fwd')
        ctx.save_for_backward(P, Q, idx, coef)
        ctx.meta = (st.train, st.G)
        return Z

    @staticmethod
    def backward(ctx, gz):
        P, Q, idx, coef = ctx.saved_tensors
        train, G = ctx.meta
        B, N, C = P.shape
        S, ns = idx.shape[1], idx.shape[2]
        gz = gz.contiguous()
        bufs = _sa_first_bwd_buffers(B, N, S, ns, C, G, gz.device)
        check(lib().sug_sa_first_bwd(_p(gz), _p(P), C, _p(Q), _p(idx), B, N, S, ns, C, G, train, _p(coef),
                                     *map(_p, bufs), _st()), 'sug_sa_first_bwd')
        dP, dQ, rf = bufs[4], bufs[5], bufs[7]
        return (dP, dQ, None) + _dgamma_dbeta(rf) + (None,)


def _sa_first_bwd_buffers(B, N, S, ns, C, G, dev):
    """The outputs and workspaces of sug_sa_first_bwd / sug_sa_first_geo_bwd, in the order both kernels take them:
    (red, off, ent, segsum, dP, dQ, ws, rf)."""
    f32 = dict(dtype=torch.float32, device=dev)
    return (torch.zeros(G + 1, 2 * C, dtype=torch.float64, device=dev),
            torch.empty(B, N + 1, dtype=torch.int32, device=dev), torch.empty(B, S * ns, dtype=torch.int32, device=dev),
            torch.empty(2, B, S, C, **f32), torch.empty(B, N, C, **f32), torch.empty(B, S, C, **f32),
            _stats_ws(C, dev), torch.empty(2 * C, **f32))


class _SAFirstLayerGeo(torch.autograd.Function):
    """relu(BN(Pf[idx] + b + Wx . (xyz[idx] - new_xyz))) over the ball-query lists (sug_sa_first_geo_fwd / bwd): the first
    layer of a set-abstraction MLP with the coordinate part taken from the difference the reference forms.  Px (= Wx . xyz
    per point) and Q (= Wx . new_xyz - b per centroid) enter only as autograd nodes: their VALUES are not read, their
    gradients (dP, dQ) route the loss to Wx and b through the ordinary linear backward."""

    @staticmethod
    def forward(ctx, Pf, Px, Q, idx, xyz, cent, Wx, bias, gamma, beta, st):
        _need_gpu(Px, Q, idx, xyz)
        idx = _i32(idx).contiguous()
        B, N, C = Px.shape
        S, ns = idx.shape[1], idx.shape[2]
        _check_groups('sa_first_layer', B, 'clouds', st.G)
        dev = Px.device
        Pfc = None if Pf is None else Pf.detach().contiguous()
        xyz, cent = xyz.detach().contiguous(), cent.detach().contiguous()
        Wxc = Wx.detach().contiguous()
        bc = None if bias is None else bias.detach().contiguous()
        g, b, coef = _bn_params(gamma, beta, st, C)
        Z = torch.empty(B, S, ns, C, dtype=torch.float32, device=dev)
        ws = _stats_ws(C, dev)
        check(lib().sug_sa_first_geo_fwd(_p(Pfc), C, _p(xyz), _p(cent), _p(Wxc), 3, _p(bc), _p(idx), B, N, S, ns, C, st.G,
                                         _p(g), _p(b), st.train, st.eps, st.momentum, _p(st.mean), _p(st.var), _p(coef), _p(Z),
                                         _p(ws), _st()), 'sug_sa_first_geo_fwd')
        saved = [idx, coef, xyz, cent, Wxc] + ([Pfc] if Pfc is not None else []) + ([bc] if bc is not None else [])
        ctx.save_for_backward(*saved)
        ctx.meta = (st.train, st.G, Pfc is not None, bc is not None, N, C)
        return Z

    @staticmethod
    def backward(ctx, gz):
        train, G, has_p, has_b, N, C = ctx.meta
        sv = list(ctx.saved_tensors)
        idx, coef, xyz, cent, Wxc = sv[:5]
        Pfc = sv[5] if has_p else None
        bc = sv[5 + int(has_p)] if has_b else None
        B, S, ns = idx.shape
        gz = gz.contiguous()
        bufs = _sa_first_bwd_buffers(B, N, S, ns, C, G, gz.device)
        check(lib().sug_sa_first_geo_bwd(_p(gz), _p(Pfc), C, _p(xyz), _p(cent), _p(Wxc), 3, _p(bc), _p(idx), B, N, S, ns, C, G,
                                         train, _p(coef), *map(_p, bufs), _st()), 'sug_sa_first_geo_bwd')
        dP, dQ, rf = bufs[4], bufs[5], bufs[7]
        # Pf and Px receive the SAME gradient tensor on purpose (y depends on them only through Pf[j] + Px-routed terms with
        # identical row gradients): both are non-leaf outputs of linear_rows whose backward only reads its upstream
        # gradient, so the alias is never written through; a clone would cost a pass over [B,N,C]
        return ((dP if has_p else None), dP, dQ, None, None, None, None, None) + _dgamma_dbeta(rf) + (None,)


SA_FIRST_GEO = _os.environ.get('SUG_SA_FIRST_GEO', '0') == '1'  # opt-in: y = Pf[j] + b + Wx.(x_j - c_s) (measured: no accuracy gain, 1 % slower)


def sa_first_layer_geo(Pf, Px, Q, idx, xyz, cent, Wx, bias, bn):
    _count_bn_call(bn)
    return _SAFirstLayerGeo.apply(Pf, Px, Q, idx, xyz, cent, Wx, bias, bn.weight, bn.bias, _bn_state(bn))


SA_FIRST = _os.environ.get('SUG_SA_FIRST', '1') != '0'          # 0: grouped tensor + GEMM (the reference's arithmetic) instead


def sa_first_layer_supported(C):
    return SA_FIRST and C in (64, 128)


def sa_first_layer(P, Q, idx, bn):
    """P [B,N,C] = W.[xyz ; feats] per point, Q [B,S,C] = Wxyz.new_xyz - b per centroid, idx [B,S,ns] ball-query
    lists -> relu(bn(P[idx] - Q)) [B,S,ns,C] (train-mode statistics over each domain group's rows)."""
    _count_bn_call(bn)
    return _SAFirstLayer.apply(P, Q, idx, bn.weight, bn.bias, _bn_state(bn))


class _LNAct(torch.autograd.Function):
    """act(LayerNorm(x)) over the rows of a small [rows, C] tensor (sug_ln_act_fwd / bwd)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, slope):
        _need_gpu(x, gamma)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        rows, C = x2.shape
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        y = torch.empty_like(x2)
        stat = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
        check(lib().sug_ln_act_fwd(_p(x2), _p(g), _p(b), rows, C, eps, float(slope), _p(y), _p(stat), _st()), 'sug_ln_act_fwd')
        ctx.save_for_backward(x2, g, b, stat)
        ctx.meta = (float(slope), tuple(x.shape))
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        x2, g, b, stat = ctx.saved_tensors
        slope, shape = ctx.meta
        rows, C = x2.shape
        gy = gy.reshape(rows, C).contiguous()
        dx, ws = torch.empty_like(x2), torch.empty_like(x2)
        dgb = torch.empty(2, C, dtype=torch.float32, device=x2.device)
        check(lib().sug_ln_act_bwd(_p(gy), _p(x2), _p(g), _p(b), _p(stat), rows, C, slope, _p(dx), _p(dgb[0]), _p(dgb[1]),
                                   _p(ws), _st()), 'sug_ln_act_bwd')
        return dx.view(shape), dgb[0], dgb[1], None, None


# The fused LayerNorm + activation of the FC heads saves 3 launches per layer on the GPU but costs more host time than
# the native ops it replaces (a Python autograd.Function per call): worth it when the step is replayed from a hipGraph
# (SUGStep(use_graph=True) switches it on), not when every launch is issued from Python.


def ln_act_supported(x, ln):
    return x.is_cuda and x.dtype == torch.float32 and x.shape[-1] <= 1024 and ln.elementwise_affine and \
        len(ln.normalized_shape) == 1 and ln.weight is not None and ln.bias is not None


def ln_act(x, ln, slope):
    """leaky_relu(ln(x), slope) for an nn.LayerNorm over the last dimension (slope 0: ReLU)."""
    return _LNAct.apply(x, ln.weight, ln.bias, ln.eps, slope)


# ---- classifier heads (Pointnet_c) in six launches ------------------------------------------------------------------
HEADS_FUSED = _os.environ.get('SUG_HEADS_FUSED', '1') != '0'       # A/B knob: 0 = library GEMMs + LayerNorm / dropout ops


def _ptrs(ts):
    """host array of device pointers (None -> null) for the per-head operands of sug_head_linear_*"""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def heads_fused_supported(heads, x):
    """Can Pointnet_c heads `heads` (1 or 2, same architecture, same input x [M, K]) run through sug_head_linear_*?"""
    if not (HEADS_FUSED and 1 <= len(heads) <= 2 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        return False
    M, K = x.shape
    L = lib()
    h0 = heads[0]
    for hd in heads:
        if hd.PTran != h0.PTran or hd.training != h0.training or hd.dropout1.p != h0.dropout1.p or hd.dropout2.p != h0.dropout2.p:
            return False
        layers = ([] if hd.PTran else [hd.mlp1]) + [hd.mlp2]
        for fc in layers:
            if len(fc.fc) != 3 or not ln_act_supported(x, fc.fc[1]) or fc.fc[1].eps != h0.mlp2.fc[1].eps:
                return False
        if type(hd.mlp2.ac) is not type(h0.mlp2.ac) or (not hd.PTran and type(hd.mlp1.ac) is not type(hd.mlp2.ac)):
            return False
        for lin in [fc.fc[0] for fc in layers] + [hd.mlp3]:
            if lin.weight.dtype != torch.float32 or not lin.weight.is_cuda:
                return False
        if hd.mlp3.weight.shape != h0.mlp3.weight.shape or hd.mlp2.fc[0].weight.shape != h0.mlp2.fc[0].weight.shape:
            return False
    dims = [K] + ([] if h0.PTran else [h0.mlp1.fc[0].out_features]) + [h0.mlp2.fc[0].out_features, h0.mlp3.out_features]
    first = (h0.mlp2 if h0.PTran else h0.mlp1).fc[0]
    if first.in_features != K or h0.mlp3.in_features != dims[-2] or (not h0.PTran and h0.mlp2.fc[0].in_features != dims[1]):
        return False
    nl = len(dims) - 1
    for i in range(nl):
        pro, epi = int(i > 0), int(i < nl - 1)
        if not L.sug_head_linear_supported(M, dims[i], dims[i + 1], pro, epi):
            return False
    return True


class _HeadsFused(torch.autograd.Function):
    """Pointnet_c heads (model/Model.py:412-449) on one input: per layer ONE launch for all heads, the LayerNorm /
    activation / dropout between two Linear layers applied to the next layer's operand as it is loaded
    (sug_head_linear_fwd); in the backward one launch per Linear layer (sug_head_linear_bwd) and one per LayerNorm
    (sug_head_ln_bwd).  Arguments after the
    scalars: per head (W1, b1, g1, be1, W2, b2, g2, be2, W3, b3) -- the first four None for the two-layer (Point
    Transformer) head.  Returns per head (logits, mid feature)."""

    @staticmethod
    def forward(ctx, x, training, p1, p2, slope, eps, nheads, *params):
        _need_gpu(x)
        assert len(params) == 10 * nheads
        P = [[None if t is None else t.detach().contiguous() for t in params[10 * h:10 * h + 10]] for h in range(nheads)]
        three = P[0][0] is not None
        x2 = x.detach().contiguous()
        M, K = x2.shape
        dev = x.device
        N1 = P[0][0].shape[0] if three else 0
        N2, NC = P[0][4].shape[0], P[0][8].shape[0]
        drop1, drop2 = training and three and p1 > 0, training and p2 > 0
        # one launch of uniform randoms for every dropout of every head: [head][M][N1 | N2]
        # (flat: [head][M][N1] blocks, then [head][M][N2] blocks -- every operand a contiguous view)
        u = torch.rand(nheads * M * (N1 + N2), dtype=torch.float32, device=dev) if (drop1 or drop2) else None
        u1 = [u[h * M * N1:(h + 1) * M * N1].view(M, N1) if drop1 else None for h in range(nheads)] if three else None
        o2 = nheads * M * N1
        u2 = [u[o2 + h * M * N2:o2 + (h + 1) * M * N2].view(M, N2) if drop2 else None for h in range(nheads)]
        H = range(nheads)
        L = lib()
        col = lambda i: [P[h][i] for h in H]
        new = lambda n: [torch.empty(M, n, dtype=torch.float32, device=dev) for _ in H]
        z1 = st1 = None
        if three:
            z1, st1 = new(N1), new(2)
            check(L.sug_head_linear_fwd(nheads, _ptrs([x2] * nheads), K, _ptrs(col(0)), _ptrs(col(1)), _ptrs(z1), None, None, None,
                                        None, None, M, K, N1, 0, slope, eps, 0.0, _st()), 'sug_head_linear_fwd')
        z2, st2, mid, logits = new(N2), new(2), new(N2), new(NC)
        if three:
            check(L.sug_head_linear_fwd(nheads, _ptrs(z1), N1, _ptrs(col(4)), _ptrs(col(5)), _ptrs(z2), _ptrs(col(2)), _ptrs(col(3)),
                                        _ptrs(u1), _ptrs(st1), None, M, N1, N2, 1, slope, eps, p1 if drop1 else 0.0, _st()),
                  'sug_head_linear_fwd')
        else:
            check(L.sug_head_linear_fwd(nheads, _ptrs([x2] * nheads), K, _ptrs(col(4)), _ptrs(col(5)), _ptrs(z2), None, None, None,
                                        None, None, M, K, N2, 0, slope, eps, 0.0, _st()), 'sug_head_linear_fwd')
        check(L.sug_head_linear_fwd(nheads, _ptrs(z2), N2, _ptrs(col(8)), _ptrs(col(9)), _ptrs(logits), _ptrs(col(6)), _ptrs(col(7)),
                                    _ptrs(u2), _ptrs(st2), _ptrs(mid), M, N2, NC, 1, slope, eps, p2 if drop2 else 0.0, _st()),
              'sug_head_linear_fwd')
        # saved through autograd (version checks, freed with the graph): parameters, then per head z1 st1 z2 st2 u1 u2, then x
        flatP = [t for h in H for t in P[h]]
        acts = []
        for h in H:
            acts += [z1[h] if three else None, st1[h] if three else None, z2[h], st2[h],
                     u1[h] if (three and u1 is not None) else None, u2[h]]
        ctx.save_for_backward(*flatP, *acts, x2)
        ctx.meta = (three, M, K, N1, N2, NC, float(slope), float(eps), float(p1 if drop1 else 0.0), float(p2 if drop2 else 0.0),
                    nheads, tuple(x.shape))
        ctx.need_dx = ctx.needs_input_grad[0]
        out = []
        for h in H:
            out += [logits[h], mid[h]]
        return tuple(out)

    @staticmethod
    def backward(ctx, *gs):
        three, M, K, N1, N2, NC, slope, eps, p1, p2, nheads, xshape = ctx.meta
        saved = ctx.saved_tensors
        H = range(nheads)
        P = [list(saved[10 * h:10 * h + 10]) for h in H]
        acts = saved[10 * nheads:10 * nheads + 6 * nheads]
        x2 = saved[-1]
        z1, st1, z2, st2, u1, u2 = ([acts[6 * h + i] for h in H] for i in range(6))
        dev = x2.device
        L = lib()
        col = lambda i: [P[h][i] for h in H]
        zeros = lambda n: torch.zeros(M, n, dtype=torch.float32, device=dev)
        gl = [gs[2 * h].contiguous() if gs[2 * h] is not None else zeros(NC) for h in H]
        gm = [None if gs[2 * h + 1] is None else gs[2 * h + 1].contiguous() for h in H]
        like = lambda i: [None if P[h][i] is None else torch.empty_like(P[h][i]) for h in H]
        new = lambda n: [torch.empty(M, n, dtype=torch.float32, device=dev) for _ in H]
        grads = [like(i) for i in range(10)]
        # layer 3: logits = Dropout(act(LN(z2))) . W3^T + b3
        da2, dz2 = new(N2), new(N2)
        check(L.sug_head_linear_bwd(nheads, 0, _ptrs(gl), NC, _ptrs(z2), N2, _ptrs(st2), _ptrs(col(6)), _ptrs(col(7)), _ptrs(u2),
                                    _ptrs(col(8)), _ptrs(grads[8]), _ptrs(grads[9]), _ptrs(da2), N2, M, N2, NC, 1, slope, p2, _st()),
              'sug_head_linear_bwd')
        check(L.sug_head_ln_bwd(nheads, _ptrs(da2), N2, _ptrs(z2), _ptrs(st2), _ptrs(col(6)), _ptrs(col(7)), _ptrs(u2), _ptrs(gm),
                                _ptrs(dz2), _ptrs(grads[6]), _ptrs(grads[7]), _ptrs(grads[5]), M, N2, slope, p2, _st()), 'sug_head_ln_bwd')
        dx = torch.empty(M, K, dtype=torch.float32, device=dev) if ctx.need_dx else None
        dxs = _ptrs([dx] + [None] * (nheads - 1))
        if three:
            da1, dz1 = new(N1), new(N1)
            check(L.sug_head_linear_bwd(nheads, 0, _ptrs(dz2), N2, _ptrs(z1), N1, _ptrs(st1), _ptrs(col(2)), _ptrs(col(3)), _ptrs(u1),
                                        _ptrs(col(4)), _ptrs(grads[4]), None, _ptrs(da1), N1, M, N1, N2, 1, slope, p1, _st()),
                  'sug_head_linear_bwd')
            check(L.sug_head_ln_bwd(nheads, _ptrs(da1), N1, _ptrs(z1), _ptrs(st1), _ptrs(col(2)), _ptrs(col(3)), _ptrs(u1), None,
                                    _ptrs(dz1), _ptrs(grads[2]), _ptrs(grads[3]), _ptrs(grads[1]), M, N1, slope, p1, _st()),
                  'sug_head_ln_bwd')
            check(L.sug_head_linear_bwd(nheads, 1, _ptrs(dz1), N1, _ptrs([x2] * nheads), K, None, None, None, None, _ptrs(col(0)),
                                        _ptrs(grads[0]), None, dxs, K, M, K, N1, 0, slope, 0.0, _st()), 'sug_head_linear_bwd')
        else:
            check(L.sug_head_linear_bwd(nheads, 1, _ptrs(dz2), N2, _ptrs([x2] * nheads), K, None, None, None, None, _ptrs(col(4)),
                                        _ptrs(grads[4]), None, dxs, K, M, K, N2, 0, slope, 0.0, _st()), 'sug_head_linear_bwd')
        flat = []
        for h in H:
            flat += [grads[i][h] for i in range(10)]
        return (None if dx is None else dx.view(xshape), None, None, None, None, None, None) + tuple(flat)


def heads_fused(heads, x):
    """[(logits, mid feature) per head] of Pointnet_c heads on the pooled feature x [M, K] (see _HeadsFused)."""
    h0 = heads[0]
    act = h0.mlp2.ac
    slope = 0.0 if isinstance(act, torch.nn.ReLU) else float(act.negative_slope)
    params = []
    for hd in heads:
        if hd.PTran:
            params += [None, None, None, None]
        else:
            params += [hd.mlp1.fc[0].weight, hd.mlp1.fc[0].bias, hd.mlp1.fc[1].weight, hd.mlp1.fc[1].bias]
        params += [hd.mlp2.fc[0].weight, hd.mlp2.fc[0].bias, hd.mlp2.fc[1].weight, hd.mlp2.fc[1].bias, hd.mlp3.weight, hd.mlp3.bias]
    out = _HeadsFused.apply(x, h0.training, float(h0.dropout1.p), float(h0.dropout2.p), slope, float(h0.mlp2.fc[1].eps),
                            len(heads), *params)
    return [(out[2 * i], out[2 * i + 1]) for i in range(len(heads))]


# ---- Point Transformer classifier head (PointTransformerCls: fc2 on points.mean(1)) in 2 + 2 launches ---------------
PTCLS_HEAD_FUSED = _os.environ.get('SUG_PTCLS_HEAD_FUSED', '1') != '0'   # A/B knob: 0 = the composed library head


def ptcls_head_supported(points, fc2):
    """Can PointTransformerCls.fc2 (Linear, ReLU, Linear, ReLU, Linear) on points [B, P, K] run through sug_ptcls_head_*?
    Otherwise the model composes the head from library ops (points.mean(1), three nn.Linear)."""
    if not (PTCLS_HEAD_FUSED and points.is_cuda and points.dtype == torch.float32 and points.dim() == 3 and len(fc2) == 5):
        return False
    l1, l2, l3 = fc2[0], fc2[2], fc2[4]
    for t in (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias):
        if t is None or not t.is_cuda or t.dtype != torch.float32:
            return False
    B, P, K = points.shape
    if l1.in_features != K or l2.in_features != l1.out_features or l3.in_features != l2.out_features:
        return False
    return bool(lib().sug_ptcls_head_supported(B, P, K, l1.out_features, l2.out_features, l3.out_features))


class _PtclsHead(torch.autograd.Function):
    """logits = L3(relu(L2(relu(L1(points.mean(1)))))) (sug_ptcls_head_fwd: 2 launches); the backward gives the gradients
    of points and of all six parameters (sug_ptcls_head_bwd: 2 launches).  Saved: the mean rows and both post-ReLU
    activations."""

    @staticmethod
    def forward(ctx, points, w1, b1, w2, b2, w3, b3):
        _need_gpu(points, w1, b1, w2, b2, w3, b3)
        p = points.detach().contiguous()
        W = [t.detach().contiguous() for t in (w1, b1, w2, b2, w3, b3)]
        B, P, K = p.shape
        N1, N2, NC = W[0].shape[0], W[2].shape[0], W[4].shape[0]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=p.device)
        mean, h1, h2, logits = new(B, K), new(B, N1), new(B, N2), new(B, NC)
        check(lib().sug_ptcls_head_fwd(_p(p), B, P, K, _p(W[0]), _p(W[1]), N1, _p(W[2]), _p(W[3]), N2, _p(W[4]), _p(W[5]), NC,
                                       _p(mean), _p(h1), _p(h2), _p(logits), _st()), 'sug_ptcls_head_fwd')
        ctx.save_for_backward(mean, h1, h2, W[0], W[2], W[4])
        ctx.P = P
        return logits

    @staticmethod
    def backward(ctx, g):
        mean, h1, h2, w1, w2, w3 = ctx.saved_tensors
        B, K = mean.shape
        P, N1, N2, NC = ctx.P, w1.shape[0], w2.shape[0], w3.shape[0]
        g = g.contiguous()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=g.device)
        dz1, dz2, dpts = new(B, N1), new(B, N2), new(B, P, K)
        dw1, db1, dw2, db2, dw3, db3 = new(N1, K), new(N1), new(N2, N1), new(N2), new(NC, N2), new(NC)
        check(lib().sug_ptcls_head_bwd(_p(g), _p(mean), _p(h1), _p(h2), B, P, K, _p(w1), N1, _p(w2), N2, _p(w3), NC,
                                       _p(dz1), _p(dz2), _p(dpts), _p(dw1), _p(db1), _p(dw2), _p(db2), _p(dw3), _p(db3), _st()),
              'sug_ptcls_head_bwd')
        return dpts, dw1, db1, dw2, db2, dw3, db3


def ptcls_head(points, w1, b1, w2, b2, w3, b3):
    """PointTransformerCls's head on the last level's features points [B, P, K] -> logits [B, NC] (see _PtclsHead)."""
    return _PtclsHead.apply(points, w1, b1, w2, b2, w3, b3)


# num_batches_tracked increments: one tiny launch per BatchNorm call unless deferred; inside a
# `deferred_bn_counts()` block they are collected and applied with one foreach add at the end.


@contextlib.contextmanager
def deferred_bn_counts():
    if CTX.pending_counts is not None:          # nested: the outer block flushes
        yield
        return
    CTX.pending_counts = {}
    try:
        yield
    finally:
        flush_bn_counts()
        CTX.pending_counts = None


def flush_bn_counts():
    """Apply the counter increments collected so far by the enclosing deferred_bn_counts() block (one multi-tensor launch,
    a scalar per counter); whoever reads num_batches_tracked inside such a block calls this first."""
    pend = CTX.pending_counts
    if pend:
        torch._foreach_add_([t for t, _ in pend.values()], [n for _, n in pend.values()])
        pend.clear()


def _count_bn_call(bn, n=None):
    if bn.training and bn.num_batches_tracked is not None:
        n = CTX.bn_groups if n is None else n
        if CTX.pending_counts is not None:
            t = bn.num_batches_tracked
            old = CTX.pending_counts.get(id(t))
            CTX.pending_counts[id(t)] = (t, n + (old[1] if old else 0))
        else:
            bn.num_batches_tracked.add_(n)


# A shared prefix (DGCNN / Point Transformer / PointNet encoders: the part of the semantic and of the node pass of a step that
# is the same computation) is run once; the second pass only REPLAYS the running-statistics updates of its BatchNorm layers.
# `with record_bn_stats() as rec:` collects (module, batch-statistics coefficients) of every train-mode BatchNorm op inside.


@contextlib.contextmanager
def record_bn_stats():
    with CTX.scoped(bn_record=[]):
        yield CTX.bn_record


def _record_bn(bn, coef):
    if CTX.bn_record is not None and bn.training and bn.track_running_stats:
        CTX.bn_record.append((bn, coef))


def replay_bn_stats(rec):
    """bn_replay for every (bn, coef) of a recorded prefix, in order; runs of distinct layers share one launch."""
    rec = list(rec)
    i = 0
    while i < len(rec):
        run, seen = [], set()
        while i < len(rec) and len(run) < 16 and id(rec[i][0]) not in seen:     # a layer recorded twice: its updates stay in order
            seen.add(id(rec[i][0]))
            run.append(rec[i])
            i += 1
        if len(run) == 1:
            bn_replay(*run[0])
            continue
        c3s = []
        for _, coef in run:
            c3 = coef if coef.dim() == 3 else coef.unsqueeze(0)
            c3s.append(c3 if c3.is_contiguous() else c3.contiguous())
        n = len(run)
        I32, F32 = ctypes.c_int32 * n, ctypes.c_float * n
        check(lib().sug_bn_replay_multi(n, _ptrs(c3s), I32(*[c.shape[0] for c in c3s]), I32(*[c.shape[2] for c in c3s]),
                                        F32(*[float(bn.momentum) for bn, _ in run]), _ptrs([bn.running_mean for bn, _ in run]),
                                        _ptrs([bn.running_var for bn, _ in run]), _st()), 'sug_bn_replay_multi')
        for (bn, _), c3 in zip(run, c3s):
            _count_bn_call(bn, c3.shape[0])


def bn_replay(bn, coef):
    """Running-statistics update of len(coef) more train-mode forwards with known batch statistics
    (coef [5,C] or [G,5,C] from a BN op), in order (sug_bn_replay)."""
    c3 = coef if coef.dim() == 3 else coef.unsqueeze(0)
    c3 = c3 if c3.is_contiguous() else c3.contiguous()
    G, _, C = c3.shape
    check(lib().sug_bn_replay(_p(c3), G, C, float(bn.momentum), _p(bn.running_mean), _p(bn.running_var), _st()),
          'sug_bn_replay')
    _count_bn_call(bn, G)


def bn_act_rows(y, bn, slope, pre=None):
    """bn: an nn.BatchNorm{1,2}d module whose parameters / running buffers are used.
    pre: (out, coef) an earlier pass of the step computed from the same y and parameters (train mode): nothing is launched,
    counted or recorded -- the caller replays the running-statistics update (replay_bn_stats)."""
    if pre is not None:
        return _BNActRows.apply(y, bn.weight, bn.bias, _bn_state(bn), slope, pre)[0]
    _count_bn_call(bn)
    out, coef = _BNActRows.apply(y, bn.weight, bn.bias, _bn_state(bn), slope)
    _record_bn(bn, coef)
    return out


# A/B knob: 0 = the bn5 stage (statistics, pooling, its backward, bn_update_stats) launches once per domain group; 1 = every
# group in each launch (sug_bn_act_pool_groups_* / sug_col_stats_bn_groups_exact), bit for bit the same results
BN_POOL_GROUPED = _os.environ.get('SUG_BN_POOL_GROUPED', '1') != '0'


class _BNActPool(torch.autograd.Function):
    """y [B,N,C] -> (max_n, mean_n) of LeakyReLU(slope)(BatchNorm(y)); one read of y forward,
    two backward (sug_bn_act_pool_*)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, st, slope):
        _need_gpu(y, gamma)
        y, B, N, C, ld = _rows3(y)
        G = st.G
        _check_groups('bn_act_pool', B, 'clouds', G)
        dev = y.device
        g, b, coef = _bn_params(gamma, beta, st, C)
        pooled = torch.empty(B, 2 * C, dtype=torch.float32, device=dev)      # [max | mean]: torch.cat((max, mean), 1) in place
        omax, omean = pooled[:, :C], pooled[:, C:]
        arg = torch.empty(B, C, dtype=torch.int32, device=dev)
        stats = torch.empty(2 * C, dtype=torch.float64, device=dev)
        grouped = BN_POOL_GROUPED and G > 1
        if grouped:                       # a statistics workspace block per group, pooling partials of all B clouds
            wss = torch.empty(G * STATS_BLOCKS * 2 * C, dtype=torch.float32, device=dev)
            wsp = torch.empty(12 * B * C, dtype=torch.float32, device=dev)
            fwd, name = lib().sug_bn_act_pool_groups_fwd, 'sug_bn_act_pool_groups_fwd'
        else:
            wss = _stats_ws(C, dev)
            wsp = torch.empty(12 * (B // G) * C, dtype=torch.float32, device=dev)
            fwd, name = lib().sug_bn_act_pool_layer_fwd, 'sug_bn_act_pool_layer_fwd'
        check(fwd(_p(y), ld, B, N, C, G, _p(g), _p(b), st.train, st.eps, st.momentum, float(slope), _p(st.mean), _p(st.var),
                  _p(coef), _p(omax), _p(omean), 2 * C, _p(arg), _p(stats), _p(wss), _p(wsp), _st()), name)
        ctx.save_for_backward(y, coef, arg)
        ctx.meta = (B, N, C, ld, float(slope), st.train, G, grouped)
        return pooled

    @staticmethod
    def backward(ctx, g):
        y, coef, arg = ctx.saved_tensors
        B, N, C, ld, slope, train, G, grouped = ctx.meta
        dev = y.device
        if g.stride(1) != 1 or g.stride(0) < 2 * C:
            g = g.contiguous()
        gmax, gmean, ldp = g[:, :C], g[:, C:], g.stride(0)
        red = torch.empty(G, 2 * C, dtype=torch.float64, device=dev)
        ws = _stats_ws(C, dev)
        dy = torch.empty(B, N, C, dtype=torch.float32, device=dev)
        rf = torch.empty(2 * C, dtype=torch.float32, device=dev)
        bwd, name = (lib().sug_bn_act_pool_groups_bwd, 'sug_bn_act_pool_groups_bwd') if grouped else \
            (lib().sug_bn_act_pool_layer_bwd, 'sug_bn_act_pool_layer_bwd')
        check(bwd(_p(y), ld, _p(coef), _p(gmax), _p(gmean), ldp, _p(arg), B, N, C, G, slope, train, _p(red), _p(ws), _p(dy), C,
                  _p(rf), _st()), name)
        return (dy,) + _dgamma_dbeta(rf) + (None, None)


def bn_update_stats(y, bn):
    """Train-mode BatchNorm side effect only: batch statistics of y [..., C] per domain group ->
    running-buffer update (and num_batches_tracked); the normalised output is not produced.  For a
    layer whose output is discarded but whose buffers the reference still updates."""
    if not bn.training:
        return
    _need_gpu(y)
    C = y.shape[-1]
    y2 = y.detach().reshape(-1, C)
    if y2.stride(1) != 1:
        y2 = y2.contiguous()
    rows, G = y2.shape[0], CTX.bn_groups
    _check_groups('bn_update_stats', rows, 'rows', G)
    rg = rows // G
    g, b = bn.weight.detach().contiguous(), bn.bias.detach().contiguous()
    if BN_POOL_GROUPED and G > 1:           # every group in one launch pair, the bits of the loop below
        coef = torch.empty(G, 5, C, dtype=torch.float32, device=y.device)
        ws = torch.empty(G * STATS_BLOCKS * 2 * C, dtype=torch.float32, device=y.device)
        check(lib().sug_col_stats_bn_groups_exact(_p(y2), y2.stride(0), rows, C, G, _p(g), _p(b), bn.eps, bn.momentum,
                                                  _p(bn.running_mean), _p(bn.running_var), _p(coef), _p(ws), _st()),
              'sug_col_stats_bn_groups_exact')
        _count_bn_call(bn)
        return
    coef = torch.empty(5, C, dtype=torch.float32, device=y.device)
    ws = _stats_ws(C, y.device)
    for i in range(G):
        yi = y2[i * rg:(i + 1) * rg]
        check(lib().sug_col_stats_bn(_p(yi), yi.stride(0), rg, C, _p(g), _p(b), bn.eps, bn.momentum,
                                     _p(bn.running_mean), _p(bn.running_var), _p(coef), _p(ws), _st()),
              'sug_col_stats_bn')
    _count_bn_call(bn)


def bn_act_pool_cat(y, bn, slope):
    """cat((max over points, mean over points), 1) [B, 2C] of act(bn(y)), y [B,N,C]: the kernels write the two halves of
    the concatenated feature (Model.py:113-116) and read the two halves of its gradient in place."""
    _count_bn_call(bn)
    return _BNActPool.apply(y, bn.weight, bn.bias, _bn_state(bn), slope)


def bn_act_pool(y, bn, slope):
    """(max over points, mean over points) of act(bn(y)), y [B,N,C]."""
    C = y.shape[-1]
    pooled = bn_act_pool_cat(y, bn, slope)
    return pooled[:, :C], pooled[:, C:]


# ----------------------------------------------------------------------------- EdgeConv
def _edgeconv_out(out_holder, B, N, Co, dev):
    """The [B,N,Co] destination of an EdgeConv layer: fresh, or the caller's (a column slice of a wider rows buffer, see
    assemble_rows; passed in a list so that autograd does not treat it as an input of the node)."""
    if out_holder is None:
        return torch.empty(B, N, Co, dtype=torch.float32, device=dev)
    out = out_holder[0]
    if tuple(out.shape) != (B, N, Co) or out.stride(2) != 1 or out.stride(0) != N * out.stride(1) \
            or out.dtype != torch.float32 or out.requires_grad:
        raise RuntimeError('edgeconv: bad destination slice')
    return out


def _edgeconv_backward(gout, z, arg, s1, pq, ldpq, idx, coef, B, N, k, Co, G, slope, train):
    """sug_edgeconv_layer_bwd from what either EdgeConv forward saved: -> (dpq [B,N,2Co], dgamma, dbeta)."""
    dev = gout.device
    gout, _, _, _, ldg = _rows3(gout)                           # a column slice of a wider buffer is fine
    a = torch.empty(B, N, Co, dtype=torch.float32, device=dev)
    # per-group dbeta | dgamma, plus a zero row the scatter reads in eval mode (statistics constant)
    red = (torch.empty if train else torch.zeros)(G + 1, 2 * Co, dtype=torch.float64, device=dev)
    ws = _stats_ws(Co, dev)
    off = torch.empty(B, N + 1, dtype=torch.int32, device=dev)
    ent = torch.empty(B, N * k, dtype=torch.int32, device=dev)
    dpq = torch.empty(B, N, 2 * Co, dtype=torch.float32, device=dev)
    rf = torch.empty(2 * Co, dtype=torch.float32, device=dev)
    check(_timed('edgeconv_layer_bwd_Co%d' % Co, {'B': B, 'N': N, 'k': k, 'Co': Co},
                 lambda: lib().sug_edgeconv_layer_bwd(_p(gout), ldg, _p(z), _p(arg), _p(s1), _p(pq), ldpq, _p(idx),
                                                      _p(coef), B, N, k, Co, G, train, slope, _p(a),
                                                      _p(red), _p(off), _p(ent), _p(dpq), 2 * Co, _p(ws), _p(rf), _st())),
          'sug_edgeconv_layer_bwd')
    return (dpq,) + _dgamma_dbeta(rf)


class _EdgeConv(torch.autograd.Function):
    """BN(train or eval) + LeakyReLU + max over k of y = P[idx] + Q, see include/sug_amd.h."""

    @staticmethod
    def forward(ctx, pq, idx, gamma, beta, st, slope, out_holder, grad_on=True):
        _need_gpu(pq, idx, gamma)
        pq, B, N, C2, ld = _rows3(pq)
        Co = C2 // 2
        idx = _i32(idx).contiguous()
        k = idx.shape[2]
        G = st.G
        _check_groups('edgeconv', B, 'clouds', G)
        dev = pq.device
        gamma_c, beta_c, coef = _bn_params(gamma, beta, st, Co)
        # (needs_input_grad reports requires_grad of the inputs even under torch.no_grad(): the caller passes the grad
        # mode, or the no-grad passes of a step would write s1 -- 4*Co bytes per point -- for a backward that never runs)
        need_bwd = grad_on and any(ctx.needs_input_grad[i] for i in (0, 2, 3))         # pq, gamma, beta
        z = torch.empty(B, N, Co, dtype=torch.float32, device=dev)
        arg = torch.empty(B, N, Co, dtype=torch.uint8, device=dev)
        s1 = torch.empty(B, N, Co, dtype=torch.float32, device=dev) if need_bwd else None
        stats = torch.empty(2 * Co, dtype=torch.float64, device=dev)
        ws = _stats_ws(Co, dev)
        out = _edgeconv_out(out_holder, B, N, Co, dev)
        ldo = out.stride(1)
        check(_timed('edgeconv_layer_fwd_Co%d' % Co, {'B': B, 'N': N, 'k': k, 'Co': Co},
                     lambda: lib().sug_edgeconv_layer_fwd(_p(pq), ld, _p(idx), _p(gamma_c), _p(beta_c), B, N, k, Co, G,
                                                          st.train, st.eps, st.momentum, float(slope),
                                                          _p(st.mean), _p(st.var), _p(z), _p(arg), _p(s1),
                                                          _p(coef), _p(out), ldo, _p(stats), _p(ws), _st())),
              'sug_edgeconv_layer_fwd')
        if need_bwd:
            ctx.save_for_backward(pq, idx, z, arg, s1, coef)
            ctx.meta = (B, N, k, Co, ld, float(slope), st.train, G)
        coef_out = coef[0] if G == 1 else coef
        ctx.mark_non_differentiable(coef_out)
        ctx.set_materialize_grads(False)
        return out, coef_out

    @staticmethod
    def backward(ctx, gout, _gcoef):
        if gout is None:
            return (None,) * 8
        pq, idx, z, arg, s1, coef = ctx.saved_tensors
        B, N, k, Co, ld, slope, train, G = ctx.meta
        dpq, dgamma, dbeta = _edgeconv_backward(gout, z, arg, s1, pq, ld, idx, coef, B, N, k, Co, G, slope, train)
        return dpq, None, dgamma, dbeta, None, None, None, None


def edgeconv_bn_act_max(pq, idx, gamma, beta, running_mean, running_var, training, slope, eps=1e-5, momentum=0.1,
                        out=None):
    """pq [B,N,2*Co] = x.[W1;W2-W1]^T, idx [B,N,k] -> (out [B,N,Co], coef [5,Co] = scale, shift,
    batch mean, rstd, unbiased batch variance; [G,5,Co] under bn_groups(G > 1))."""
    return _EdgeConv.apply(pq, idx, gamma, beta, _BNState(running_mean, running_var, training, eps, momentum), slope,
                           None if out is None else [out], torch.is_grad_enabled())


def edgeconv_path(backward, B, N, k, Co):
    """True where the LDS-resident kernel takes the shape, False where the generic one does: the forward gather / reduce
    of edgeconv_bn_act_max over B clouds (those of one group where the layer runs group by group), or with `backward` the
    scatter of the backward of either EdgeConv layer.  The dispatch's own condition (sug_edgeconv_path), alignment aside."""
    return bool(lib().sug_edgeconv_path(int(bool(backward)), B, N, k, Co))


# The 1x1 convolution inside the gather kernel (edgeconv_fused.hip): default; SUG_EDGECONV_FUSED=0 selects the
# library GEMM + edgeconv_bn_act_max path (A/B measurements).
EDGECONV_FUSED = _os.environ.get('SUG_EDGECONV_FUSED', '1') == '1'


# Widest input the fused layer takes by default.  A workgroup = (cloud, 16-channel slice) streams the cloud's x rows
# through L2 once per slice; at Cin = 128 / Co = 256 (DGCNN conv4: 16 slices x 512 KB per cloud) those re-reads cost
# more than the [P|Q] round trip of the library-GEMM path (tools/bench_edgeconv_fused.py: 208 vs ~190 us per 64 clouds),
# at Cin <= 64 the fused layer is level or ahead.  SUG_EDGECONV_FUSED_MAXC=128 fuses every layer.
EDGECONV_FUSED_MAXC = int(_os.environ.get('SUG_EDGECONV_FUSED_MAXC', '64'))


def edgeconv_fused_supported(N, k, Cin, Co):
    return EDGECONV_FUSED and Cin <= EDGECONV_FUSED_MAXC and bool(lib().sug_edgeconv_fused_supported(N, k, Cin, Co))


class _EdgeConvFused(torch.autograd.Function):
    """max_k LeakyReLU(BN(W.[x_j - x_i ; x_i])) from the rows x and the split weight [W1 ; W2-W1]: the GEMM, the
    neighbour gather, the reduction over k and the BatchNorm sums in one kernel, BatchNorm + activation in a second
    (sug_edgeconv_fused_layer_fwd).  [P|Q] is written only for a backward (sug_edgeconv_layer_bwd reads it)."""

    @staticmethod
    def forward(ctx, x, wcat, bias, idx, gamma, beta, st, slope, out_holder, grad_on=True):
        _need_gpu(x, wcat, idx, gamma)
        x3, B, N, C, ld = _rows3(x)
        Co = wcat.shape[0] // 2
        idx = _i32(idx).contiguous()
        k = idx.shape[2]
        G = st.G
        _check_groups('edgeconv', B, 'clouds', G)
        dev = x.device
        w = wcat.detach().contiguous()
        b1 = None if bias is None else bias.detach().contiguous()
        gamma_c, beta_c, coef = _bn_params(gamma, beta, st, Co)
        # (needs_input_grad ignores torch.no_grad(): the caller passes the grad mode -- see _EdgeConv)
        need_bwd = grad_on and any(ctx.needs_input_grad[i] for i in (0, 1, 2, 4, 5))   # x, wcat, bias, gamma, beta
        z = torch.empty(B, N, Co, dtype=torch.float32, device=dev)
        arg = torch.empty(B, N, Co, dtype=torch.uint8, device=dev) if need_bwd else None
        s1 = torch.empty(B, N, Co, dtype=torch.float32, device=dev) if need_bwd else None
        pq = torch.empty(B, N, 2 * Co, dtype=torch.float32, device=dev) if need_bwd else None
        ws = _stats_ws(Co, dev)
        out = _edgeconv_out(out_holder, B, N, Co, dev)
        check(_timed('edgeconv_fused_fwd_C%d_Co%d' % (C, Co), {'B': B, 'N': N, 'k': k, 'Co': Co, 'C': C, 'train': int(need_bwd)},
                     lambda: lib().sug_edgeconv_fused_layer_fwd(_p(x3), ld, C, _p(w), _p(b1), _p(idx), _p(gamma_c), _p(beta_c),
                                                                B, N, k, Co, G, st.train, st.eps, st.momentum,
                                                                float(slope), _p(st.mean), _p(st.var), _p(z),
                                                                _p(arg), _p(s1), _p(pq), 2 * Co, _p(coef), _p(out),
                                                                out.stride(1), _p(ws), _st())),
              'sug_edgeconv_fused_layer_fwd')
        if need_bwd:
            ctx.save_for_backward(x3, w, idx, z, arg, s1, coef, pq)
            ctx.meta = (B, N, k, C, Co, float(slope), st.train, G, b1 is not None, tuple(x.shape))
        coef_out = coef[0] if G == 1 else coef
        ctx.mark_non_differentiable(coef_out)
        ctx.set_materialize_grads(False)
        return out, coef_out

    @staticmethod
    def backward(ctx, gout, _gcoef):
        if gout is None:
            return (None,) * 10
        x3, w, idx, z, arg, s1, coef, pq = ctx.saved_tensors
        B, N, k, C, Co, slope, train, G, has_bias, xshape = ctx.meta
        dpq, dgamma, dbeta = _edgeconv_backward(gout, z, arg, s1, pq, 2 * Co, idx, coef, B, N, k, Co, G, slope, train)
        x2 = x3.reshape(B * N, C) if x3.is_contiguous() else x3.view(B * N, C) if x3.stride(0) == N * x3.stride(1) else x3.reshape(B * N, C)
        dpq2 = dpq.view(B * N, 2 * Co)
        dx, dw, _ = linear_rows_backward(x2, w, dpq2, ctx.needs_input_grad[0], ctx.needs_input_grad[1], False)
        db = None
        if has_bias and ctx.needs_input_grad[2]:
            db = colsum(dpq2[:, Co:])                              # the bias rides on the Q half
        return (None if dx is None else dx.view(xshape)), dw, db, None, dgamma, dbeta, None, None, None, None


def edgeconv_fused(x, wcat, bias, idx, bn_weight, bn_bias, running_mean, running_var, training, slope, eps=1e-5,
                   momentum=0.1, out=None):
    """x [B,N,C] rows, wcat [2Co, C] = [W1 ; W2-W1], idx [B,N,k] -> (out [B,N,Co], coef) as edgeconv_bn_act_max."""
    return _EdgeConvFused.apply(x, wcat, bias, idx, bn_weight, bn_bias,
                                _BNState(running_mean, running_var, training, eps, momentum), slope,
                                None if out is None else [out], torch.is_grad_enabled())


# ----------------------------------------------------------------------------- per-point MLP + max
POINTMLP_MAX = _os.environ.get('SUG_POINTMLP_MAX', '1') != '0'    # 0: library GEMM + BatchNorm rows kernels + torch.max instead


def pointmlp_max_supported(K, Co, seg):
    return POINTMLP_MAX and K in (64, 128) and Co % 128 == 0 and seg >= 32 and seg % 32 == 0


class _PointMLPMax(torch.autograd.Function):
    """max over `seg` consecutive rows of act(BN(x . W^T + b)) without ever storing the [rows, Co]
    product (sug_pointmlp_max_*).  Backward: the rows that won a channel get a[s,c]*W[c,:]
    (sug_pointmlp_max_bwd_sparse); the train-mode BatchNorm statistics terms, which are dense over the
    rows but of rank K, are -(x.A + v) with A = W^T diag(k2) W -- one [rows,K]x[K,K] GEMM instead of
    the [rows,Co]x[Co,K] one -- and the matching weight-gradient term comes from X^T X."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, st, slope, seg):
        _need_gpu(x, weight, gamma)
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        if x2.stride(1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        rows, Co = x2.shape[0], weight.shape[0]
        _check_groups('pointmlp_max', rows, 'rows', st.G, seg)
        S = rows // seg
        dev = x.device
        w2 = weight.detach().reshape(Co, K).contiguous()
        b1 = None if bias is None else bias.detach().contiguous()
        g, b, coef = _bn_params(gamma, beta, st, Co)
        zext = torch.empty(S, Co, dtype=torch.float32, device=dev)
        arg = torch.empty(S, Co, dtype=torch.int32, device=dev)
        out = torch.empty(S, Co, dtype=torch.float32, device=dev)
        ws = _stats_ws(Co, dev)
        check(_timed('pointmlp_max_K%d_Co%d' % (K, Co), {'B': rows, 'N': seg, 'k': K, 'Co': Co},
                     lambda: lib().sug_pointmlp_max_layer_fwd(_p(x2), x2.stride(0), rows, K, _p(w2), _p(b1), _p(g), _p(b),
                                                              Co, seg, st.G, st.train, st.eps, st.momentum,
                                                              float(slope), _p(st.mean), _p(st.var), _p(zext),
                                                              _p(arg), _p(coef), _p(out), Co, _p(ws), _st())),
              'sug_pointmlp_max_layer_fwd')
        if any(ctx.needs_input_grad[i] for i in (0, 1, 2, 3, 4)):       # x, weight, bias, gamma, beta
            ctx.save_for_backward(x2, w2, b1, zext, arg, coef)
            ctx.meta = (rows, K, Co, seg, st.G, float(slope), st.training, tuple(x.shape), tuple(weight.shape))
        ctx.mark_non_differentiable(coef)
        ctx.set_materialize_grads(False)
        return out, coef

    @staticmethod
    def backward(ctx, gout, _gcoef):
        x2, w2, b1, zext, arg, coef = ctx.saved_tensors
        rows, K, Co, seg, G, slope, training, xshape, wshape = ctx.meta
        if gout is None:                    # an undefined gradient counts as zeros, as if autograd had materialised it
            gout = torch.zeros_like(zext)
        dx, dw, db, dgamma, dbeta = _pointmlp_max_backward(gout, x2, w2, b1, zext, arg, coef, rows, K, Co, seg, G, slope, training)
        return dx.view(xshape), dw.view(wshape), db, dgamma, dbeta, None, None, None


def _pointmlp_max_backward(gout, x2, w2, b1, zext, arg, coef, rows, K, Co, seg, G, slope, training):
    """Backward of the fused per-point MLP + max layer (see _PointMLPMax): -> (dx [rows, K], dw [Co, K], db, dgamma, dbeta)."""
    dev = gout.device
    S = rows // seg
    rg, sg = rows // G, S // G
    gout = gout.reshape(S, Co)
    if gout.stride(1) != 1 or gout.stride(0) % 4 or gout.data_ptr() % 16:
        gout = gout.contiguous()        # e.g. a column slice of a [.., 3 + C] gradient: the float4 kernels need aligned rows
    a = torch.empty(S, Co, dtype=torch.float32, device=dev)
    red = torch.empty(G, 2 * Co, dtype=torch.float64, device=dev)
    ws = _stats_ws(Co, dev)
    dx = torch.empty(rows, K, dtype=torch.float32, device=dev) if training else \
        torch.zeros(rows, K, dtype=torch.float32, device=dev)
    # dw (accumulated over the groups) and the identically-zero bias gradient of a train-mode layer: ONE zero fill
    zdb = Co if (b1 is not None and training) else 0
    zbuf = torch.zeros(Co * K + zdb, dtype=torch.float32, device=dev)
    dw = zbuf[:Co * K].view(Co, K)
    dws = torch.empty(Co, K, dtype=torch.float32, device=dev)
    wsp = torch.empty(int(lib().sug_pointmlp_max_bwd_workspace(rg, K, Co, seg)), dtype=torch.float32, device=dev)
    L = lib()
    f32 = dict(dtype=torch.float32, device=dev)
    kbk2, negA, negv = torch.empty(2, Co, **f32), torch.empty(K, K, **f32), torch.empty(K, **f32)
    nkb, nwk = torch.empty(Co, **f32), torch.empty(Co, K, **f32)
    xtx, sx = torch.empty(K, K, **f32), torch.empty(K, **f32)
    wsx = torch.empty(int(L.sug_linear_dw_workspace(rg, K, K)), **f32) if training else None
    for gi in range(G):
        xg = x2[gi * rg:(gi + 1) * rg]
        zg, ag, cg = zext[gi * sg:(gi + 1) * sg], a[gi * sg:(gi + 1) * sg], coef[gi]
        gg = gout[gi * sg:(gi + 1) * sg]
        check(L.sug_edgeconv_bwd_reduce(_p(gg), gg.stride(0), _p(zg), _p(cg), sg, Co, slope, _p(ag), _p(red[gi]), _p(ws),
                                        _st()), 'sug_edgeconv_bwd_reduce')
        dxg = dx[gi * rg:(gi + 1) * rg]
        if training:
            # dy = a_full - (scale/M)(dbeta + xhat*dgamma) = a_full - k1 - k2*y over ALL rows, y = x.W^T + b:
            # the coefficients kb, k2 and the operands of -A, -v from one launch (sug_pointmlp_max_bwd_coef)
            check(L.sug_pointmlp_max_bwd_coef(_p(cg), _p(red[gi]), _p(b1), _p(w2), rg, K, Co, _p(kbk2[0]), _p(kbk2[1]),
                                              _p(nkb), _p(nwk), _st()), 'sug_pointmlp_max_bwd_coef')
            torch.mm(nwk.t(), w2, out=negA)                         # -A = -(W^T diag(k2) W)   [K,K]
            torch.mv(w2.t(), nkb, out=negv)                         # -v = -(kb . W)           [K]
            check(L.sug_linear_dw_bias(_p(xg), xg.stride(0), _p(xg), xg.stride(0), rg, K, K, _p(xtx), _p(sx), _p(wsx),
                                       _st()), 'sug_linear_dw_bias')        # X^T X and the column sums of x
            # -(x.A + v): alpha = beta = 1 keeps the library's bias epilogue (any other alpha first expands
            # the bias into dx: a full extra pass)
            torch.addmm(negv, xg, negA, out=dxg)
        check(L.sug_pointmlp_max_bwd_sparse(_p(ag), _p(arg[gi * sg:(gi + 1) * sg]), _p(xg), xg.stride(0), _p(w2), rg, K,
                                            Co, seg, _p(dxg), K, _p(dws), _p(wsp), _st()),
              'sug_pointmlp_max_bwd_sparse')
        check(L.sug_pointmlp_max_bwd_dwfix(_p(dw), _p(dws), _p(kbk2[0]), _p(kbk2[1]), _p(w2), _p(xtx), _p(sx), K, Co,
                                           int(training), _st()), 'sug_pointmlp_max_bwd_dwfix')
    rf = torch.empty(2 * Co, dtype=torch.float32, device=dev)
    check(L.sug_fold_groups(_p(red), G, 2 * Co, _p(rf), _st()), 'sug_fold_groups')      # dbeta | dgamma over the groups, in group order
    db = None
    if b1 is not None:
        # a bias in front of train-mode BatchNorm has zero gradient identically
        db = zbuf[Co * K:].view_as(b1) if training else a.sum(dim=0)
    return (dx, dw, db) + _dgamma_dbeta(rf)


def pointmlp_max(x, weight, bias, bn, slope, seg):
    """x [..., K] rows (segments of `seg` consecutive rows), weight [Co, K(,1,1)], bn an nn.BatchNorm
    module -> [rows/seg, Co] = max over each segment of LeakyReLU_slope(bn(x.W^T + b))."""
    _count_bn_call(bn)
    out, coef = _PointMLPMax.apply(x, weight, bias, bn.weight, bn.bias, _bn_state(bn), slope, seg)
    _record_bn(bn, coef)
    return out


# The middle layer of a set-abstraction MLP folded into the fused last layer (round 5): the middle layer's BatchNorm + ReLU is
# applied by sug_pointmlp_max_layer_fwd_xf to its x operand on the way into LDS, the activated tensor z is written once as a
# side output (only when a backward or the SA-node features need it) -- instead of a separate pass that reads y and writes z
# followed by the last layer's read of z.  SUG_SA_MID_FUSED=0 restores the separate BatchNorm pass (A/B).
SA_MID_FUSED = _os.environ.get('SUG_SA_MID_FUSED', '1') != '0'


class _BNActPointMLPMax(torch.autograd.Function):
    """(max over `seg` rows of act2(BN2(z . W^T + b)), z) with z = act1(BN1(y)) formed inside the kernel from the
    pre-activation rows y [rows, K] of the previous layer (pointnet2_utils.py:193-207: mlp_bns[i] / relu of layer i, conv /
    bn / relu / max of layer i + 1).  Outputs: out [rows/seg, Co] and z [rows, K] (None unless wanted).  Backward = the two
    layers' backward kernels unchanged: _pointmlp_max_backward on (z, gout), the gradient arriving at z added, then
    _bn_act_rows_backward through BN1."""

    @staticmethod
    def forward(ctx, y, g1, be1, weight, bias, g2, be2, st1, slope1, st2, slope2, seg, want_z, last_grad, grad_on):
        _need_gpu(y, weight, g1, g2)
        K = y.shape[-1]
        y2 = y.reshape(-1, K)
        if y2.stride(1) != 1 or y2.stride(0) != K or y2.data_ptr() % 16:
            y2 = y2.contiguous()
        rows, Co = y2.shape[0], weight.shape[0]
        G, training = st1.G, st1.training                   # one mode for both layers: bn_act_pointmlp_max checks it
        _check_groups('bn_act_pointmlp_max', rows, 'rows', G, seg)
        S = rows // seg
        dev = y.device
        L = lib()
        g1c, be1c, coef1 = _bn_params(g1, be1, st1, K)
        ws = _stats_ws(max(K, Co), dev)
        if training:
            check(L.sug_col_stats_bn_grouped(_p(y2), K, rows, K, G, _p(g1c), _p(be1c), st1.eps, st1.momentum, _p(st1.mean),
                                             _p(st1.var), _p(coef1), _p(ws), _st()), 'sug_col_stats_bn_grouped')
        need1 = grad_on and any(ctx.needs_input_grad[i] for i in (0, 1, 2))             # y, g1, be1
        need2 = grad_on and last_grad and (need1 or any(ctx.needs_input_grad[i] for i in (3, 4, 5, 6)))  # weight, bias, g2, be2
        z = torch.empty(rows, K, dtype=torch.float32, device=dev) if (want_z or need2) else None
        w2 = weight.detach().reshape(Co, K).contiguous()
        b1 = None if bias is None else bias.detach().contiguous()
        g2c, be2c, coef2 = _bn_params(g2, be2, st2, Co)
        zext = torch.empty(S, Co, dtype=torch.float32, device=dev)
        arg = torch.empty(S, Co, dtype=torch.int32, device=dev)
        out = torch.empty(S, Co, dtype=torch.float32, device=dev)
        check(_timed('pointmlp_max_K%d_Co%d' % (K, Co), {'B': rows, 'N': seg, 'k': K, 'Co': Co},
                     lambda: L.sug_pointmlp_max_layer_fwd_xf(_p(y2), K, rows, K, _p(coef1), float(slope1), _p(z), K, _p(w2), _p(b1),
                                                             _p(g2c), _p(be2c), Co, seg, G, st2.train, st2.eps, st2.momentum,
                                                             float(slope2), _p(st2.mean), _p(st2.var), _p(zext), _p(arg),
                                                             _p(coef2), _p(out), Co, _p(ws), _st())),
              'sug_pointmlp_max_layer_fwd_xf')
        ctx.need1, ctx.need2 = need1, need2
        if need1 or need2:
            ctx.save_for_backward(y2, coef1, z, w2, b1, zext, arg, coef2)
            ctx.meta = (rows, K, Co, seg, G, float(slope1), float(slope2), training, tuple(y.shape), tuple(weight.shape))
        ctx.mark_non_differentiable(*((coef1, coef2) if last_grad else (coef1, coef2, out)))
        ctx.set_materialize_grads(False)
        return out, (None if z is None else z.view(y.shape)), coef1, coef2

    @staticmethod
    def backward(ctx, gout, gz, _gcoef1, _gcoef2):
        if not (ctx.need1 or ctx.need2):
            # nothing was saved: neither the input nor any parameter of the two layers takes a gradient (a gradient that
            # still arrives at z -- want_z with the layers frozen -- has nowhere to go)
            return (None,) * 15
        y2, coef1, z, w2, b1, zext, arg, coef2 = ctx.saved_tensors
        rows, K, Co, seg, G, slope1, slope2, training, yshape, wshape = ctx.meta
        dz = dw = db = dg2 = db2 = None
        if ctx.need2 and gout is not None:
            dz, dw, db, dg2, db2 = _pointmlp_max_backward(gout, z, w2, b1, zext, arg, coef2, rows, K, Co, seg, G, slope2, training)
            dw = dw.view(wshape)
        if gz is not None:                                    # the SA-node features' gradient arrives at z too
            gz2 = gz.reshape(rows, K)
            dz = gz2 if dz is None else dz.add_(gz2)
        dy = dg1 = db1 = None
        if ctx.need1 and dz is not None:
            dy, dg1, db1 = _bn_act_rows_backward(dz, y2, coef1, rows, K, slope1, training, G)
            dy = dy.view(yshape)
        return dy, dg1, db1, dw, db, dg2, db2, None, None, None, None, None, None, None, None


def bn_act_pointmlp_max(y, bn1, slope1, weight, bias, bn2, slope2, seg, want_z=False, last_grad=True):
    """y [..., K] = pre-activation rows of the layer in front -> (max over `seg`-row segments of act2(bn2(z.W^T + b)), z or
    None) with z = act1(bn1(y)) never read back from memory by the last layer (see _BNActPointMLPMax)."""
    if bn1.training != bn2.training:
        # one `training` flag drives both BatchNorms of the fused pair (batch statistics + buffer update, or running
        # statistics): a frozen BatchNorm beside a training one has no fused form -- the callers
        # (conv_2d.rows_max_after, PointNetSetAbstraction) compare the modes and take the layer-by-layer path
        raise RuntimeError('bn_act_pointmlp_max: the two BatchNorm layers must be in the same mode (train / eval)')
    _count_bn_call(bn1)
    _count_bn_call(bn2)
    out, z, coef1, coef2 = _BNActPointMLPMax.apply(y, bn1.weight, bn1.bias, weight, bias, bn2.weight, bn2.bias, _bn_state(bn1),
                                                   slope1, _bn_state(bn2), slope2, seg, want_z, last_grad,
                                                   torch.is_grad_enabled())
    _record_bn(bn1, coef1)                             # a shared prefix replays these running-statistics updates (record_bn_stats)
    _record_bn(bn2, coef2)
    return out, z


# ----------------------------------------------------------------------------- two-layer EdgeConv block
# The EdgeConv block with two 1x1 convolutions in front of the max over k (DGCNN part segmentation, transform_net's DGCNN
# form): sug_edge_expand_fwd + sug_edgemlp_max_layer_fwd_xf.  SUG_EDGE2_FUSED=0 selects the composed form below (A/B).
EDGE2_FUSED = _os.environ.get('SUG_EDGE2_FUSED', '1') != '0'


def edgeconv2_supported(k, C1, Co):
    return EDGE2_FUSED and bool(lib().sug_edgemlp_supported(int(k), int(C1), int(Co)))


class _EdgeConv2(torch.autograd.Function):
    """out [B,N,Co] = act2(BN2(ext_j (act1(BN1(P[idx] + Q)) . W^T + b))) from pq [B,N,2*C1] = [P | Q] and idx [B,N,k].
    Forward: y1 written once with the BatchNorm-1 sums (sug_edge_expand_fwd); a1 formed on y1's way into LDS and written
    once when a backward follows; y2 exists only as accumulator tiles (sug_edgemlp_max_layer_fwd_xf).  Backward = the
    pieces of _BNActPointMLPMax unchanged -- _pointmlp_max_backward on (a1, gout) with seg = k, _bn_act_rows_backward
    through BN1 -- then sug_edge_expand_bwd folds dY1 into [dP | dQ] over the reverse lists."""

    @staticmethod
    def forward(ctx, pq, idx, g1, be1, weight, bias, g2, be2, st1, slope1, st2, slope2, out_holder, grad_on):
        _need_gpu(pq, idx, weight, g1, g2)
        pq, B, N, C2, ld = _rows3(pq)
        if ld % 4 or pq.data_ptr() % 16:
            pq, ld = pq.contiguous(), C2
        C1 = C2 // 2
        idx = _i32(idx).contiguous()
        k = idx.shape[2]
        Co = weight.shape[0]
        rows = B * N * k
        dev = pq.device
        L = lib()
        training = st1.training
        g1c, be1c, coef1 = _bn_params(g1, be1, st1, C1)
        g2c, be2c, coef2 = _bn_params(g2, be2, st2, Co)
        ws = _stats_ws(max(C1, Co), dev)
        y1 = torch.empty(rows, C1, dtype=torch.float32, device=dev)
        check(L.sug_edge_expand_fwd(_p(pq), ld, _p(idx), B, N, k, C1, _p(g1c), _p(be1c), st1.train, st1.eps, st1.momentum,
                                    _p(st1.mean), _p(st1.var), _p(y1), _p(coef1), _p(ws), _st()), 'sug_edge_expand_fwd')
        need_bwd = grad_on and any(ctx.needs_input_grad[i] for i in (0, 2, 3, 4, 5, 6, 7))
        z = torch.empty(rows, C1, dtype=torch.float32, device=dev) if need_bwd else None
        w2 = weight.detach().reshape(Co, C1).contiguous()
        b1 = None if bias is None else bias.detach().contiguous()
        zext = torch.empty(B * N, Co, dtype=torch.float32, device=dev)
        arg = torch.empty(B * N, Co, dtype=torch.int32, device=dev)
        out = _edgeconv_out(out_holder, B, N, Co, dev)
        check(_timed('edgemlp_max_Co%d' % Co, {'B': B, 'N': N, 'k': k, 'Co': Co},
                     lambda: L.sug_edgemlp_max_layer_fwd_xf(_p(y1), C1, rows, C1, _p(coef1), float(slope1), _p(z), C1, _p(w2),
                                                            _p(b1), _p(g2c), _p(be2c), Co, k, 1, st2.train, st2.eps,
                                                            st2.momentum, float(slope2), _p(st2.mean), _p(st2.var), _p(zext),
                                                            _p(arg), _p(coef2), _p(out), out.stride(1), _p(ws), _st())),
              'sug_edgemlp_max_layer_fwd_xf')
        if need_bwd:
            ctx.save_for_backward(idx, y1, coef1, z, w2, b1, zext, arg, coef2)
            ctx.meta = (B, N, k, C1, Co, float(slope1), float(slope2), training, tuple(weight.shape))
        ctx.need_bwd = need_bwd
        ctx.mark_non_differentiable(coef1, coef2)
        ctx.set_materialize_grads(False)
        return out, coef1, coef2

    @staticmethod
    def backward(ctx, gout, _gcoef1, _gcoef2):
        if gout is None or not ctx.need_bwd:
            return (None,) * 14
        idx, y1, coef1, z, w2, b1, zext, arg, coef2 = ctx.saved_tensors
        B, N, k, C1, Co, slope1, slope2, training, wshape = ctx.meta
        rows = B * N * k
        gout = gout.reshape(B * N, Co)
        dz, dw, db, dg2, db2 = _pointmlp_max_backward(gout, z, w2, b1, zext, arg, coef2, rows, C1, Co, k, 1, slope2, training)
        dy1, dg1, db1 = _bn_act_rows_backward(dz, y1, coef1, rows, C1, slope1, training, 1)
        dpq = None
        if ctx.needs_input_grad[0]:
            off, ent = knn_reverse(idx)
            dpq = torch.empty(B, N, 2 * C1, dtype=torch.float32, device=gout.device)
            check(lib().sug_edge_expand_bwd(_p(dy1), _p(off), _p(ent), B, N, k, C1, _p(dpq), 2 * C1, _st()), 'sug_edge_expand_bwd')
        return (dpq, None, dg1, db1, dw.view(wshape), db, dg2, db2) + (None,) * 6


class _EdgeExpandLists(torch.autograd.Function):
    """y1 = P[idx] + Q of the composed block for lists with more entries per cloud than the ordered scatter behind
    gather_rows' backward takes (sug_scatter_rows_ordered_supported): the same forward; the backward over sug_knn_reverse's
    lists (sug_edge_expand_bwd: one fixed order, the same bits run to run) where gather_rows would add with atomics."""

    @staticmethod
    def forward(ctx, pq, idx):
        C1 = pq.shape[-1] // 2
        idx = _i32(idx).contiguous()
        ctx.save_for_backward(idx)
        ctx.shape = (pq.shape[0], pq.shape[1], C1)
        return gather_rows(pq[:, :, :C1], idx) + pq[:, :, C1:].unsqueeze(2)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, N, C1 = ctx.shape
        g = g.contiguous()
        off, ent = knn_reverse(idx)
        dpq = torch.empty(B, N, 2 * C1, dtype=torch.float32, device=g.device)
        check(lib().sug_edge_expand_bwd(_p(g), _p(off), _p(ent), B, N, idx.shape[2], C1, _p(dpq), 2 * C1, _st()),
              'sug_edge_expand_bwd')
        return dpq, None


def _edgeconv2_composed(pq, idx, bn1, slope1, weight, bias, bn2, slope2):
    """The block from the single-layer ops, every k-expanded tensor stored: y1 (gather + add), a1, y2, a2, then torch.max."""
    B, N, C1 = pq.shape[0], pq.shape[1], pq.shape[-1] // 2
    k = idx.shape[2]
    if SCATTER_ORDERED and C1 == 64 and k <= 32 and not lib().sug_scatter_rows_ordered_supported(B, N, N * k):
        y1 = _EdgeExpandLists.apply(pq, idx)
    else:
        y1 = gather_rows(pq[:, :, :C1], idx) + pq[:, :, C1:].unsqueeze(2)    # [B,N,k,C1]
    a1 = bn_act_rows(y1, bn1, slope1)
    a2 = bn_act_rows(linear_rows(a1, weight.reshape(weight.shape[0], C1), bias), bn2, slope2)
    return a2.max(dim=2)[0]


def edgeconv2(pq, idx, bn1, slope1, weight, bias, bn2, slope2, out=None):
    """pq [B,N,2*C1] = x . [W1 ; W2-W1]^T (bias on the Q half, as conv_2d.edge_rows forms it), idx [B,N,k], bn1 / bn2
    nn.BatchNorm modules, weight [Co, C1(,1,1)] -> [B,N,Co] = max over the k neighbours of
    LeakyReLU_slope2(bn2(LeakyReLU_slope1(bn1(P[idx] + Q)) . W^T + b)).  out: a [B,N,Co] column slice to write into.
    Shapes outside edgeconv2_supported (or SUG_EDGE2_FUSED=0) run the composed GPU form."""
    _need_gpu(pq, idx, weight)
    if bn1.training != bn2.training:
        raise RuntimeError('edgeconv2: the two BatchNorm layers must be in the same mode (train / eval)')
    if CTX.bn_groups != 1:
        raise RuntimeError('edgeconv2: one domain group only (got bn_groups = %d)' % CTX.bn_groups)
    if pq.dim() != 3 or idx.dim() != 3 or pq.shape[:2] != idx.shape[:2] or pq.shape[2] % 2 or \
            weight.reshape(weight.shape[0], -1).shape[1] * 2 != pq.shape[2]:
        raise RuntimeError('edgeconv2: pq [B,N,2*C1], idx [B,N,k], weight [Co,C1] (got %s, %s, %s)'
                           % (tuple(pq.shape), tuple(idx.shape), tuple(weight.shape)))
    if not edgeconv2_supported(idx.shape[2], pq.shape[2] // 2, weight.shape[0]):
        res = _edgeconv2_composed(pq, idx, bn1, slope1, weight, bias, bn2, slope2)
        if out is not None:
            res = assemble_rows(out, (res,)) if out.shape == res.shape else res
        return res
    _count_bn_call(bn1)
    _count_bn_call(bn2)
    res, coef1, coef2 = _EdgeConv2.apply(pq, idx, bn1.weight, bn1.bias, weight, bias, bn2.weight, bn2.bias, _bn_state(bn1),
                                         slope1, _bn_state(bn2), slope2, None if out is None else [out],
                                         torch.is_grad_enabled())
    _record_bn(bn1, coef1[0])
    _record_bn(bn2, coef2[0])
    return res


# Step-scoped cache of 16-bit copies of weights / biases (opt-in: SUGStep sets a dict before the forwards of a step and
# drops it after them).  Without it every call re-casts its operands: ~280 tiny launches per step at config 5.


def cast_cached(p, lo, detach=False):
    """16-bit copy of a parameter; shared by the calls of one step when the cache is on.  Attached copies
    (detach=False) stay in the autograd graph: the fp32 parameter receives the sum of their gradients."""
    if p is None:
        return None
    if CTX.w16_cache is None:
        return (p.detach() if detach else p).to(lo)
    key = (id(p), lo, bool(detach) or not torch.is_grad_enabled())
    hit = CTX.w16_cache.get(key)
    if hit is None or hit[0] != p._version:
        hit = (p._version, (p.detach() if key[2] else p).to(lo), p)
        CTX.w16_cache[key] = hit
    return hit[1]


def w16_plan(cache):
    """The detached copies a step made, as (key, parameter, buffer) records: the next step refreshes all the buffers
    with one multi-tensor copy (w16_prefill) instead of one cast launch per parameter."""
    return [(key, hit[2], hit[1]) for key, hit in cache.items() if key[2]]


def w16_prefill(plan):
    """A cache for this step whose planned entries are already current."""
    if plan:
        torch._foreach_copy_([buf for _, _, buf in plan], [p.detach() for _, p, _ in plan])
    return {key: (p._version, buf, p) for key, p, buf in plan}


@contextlib.contextmanager
def w16_scope(holder, slot):
    """The forwards of one step (or of one phase of it) share their 16-bit weight copies; `holder[slot]` keeps the plan from
    one block to the next, so that from the second on all copies are refreshed by one multi-tensor copy into the first's
    buffers.  Off (no cache) outside the Point Transformer's 16-bit mode."""
    from .model import Ptran_transformer as _PT
    CTX.w16_cache = w16_prefill(holder[slot] or []) if _PT.GEMM_DTYPE is not None else None
    try:
        yield
    finally:
        if CTX.w16_cache is not None:
            holder[slot] = w16_plan(CTX.w16_cache)
        CTX.w16_cache = None


def _dweight(gy, x):
    """gy^T . x over the R rows in row chunks (batched GEMM = split-K: one [M,K] product alone fills few
    workgroups), chunk results summed in fp32; 16-bit operands give fp32 products straight out of the GEMM."""
    f32 = torch.float32
    R = gy.shape[0]
    # ~32 chunks (x 4 output tiles of the library's 256 x 256 macro tile = half the chip's workgroup slots), chunks of
    # 512 .. 16384 rows: R = 2^20 -> 64 x 16384, 2^17 -> 32 x 4096, 2^15 -> 32 x 1024, 2^13 -> 16 x 512
    S = 1
    while R % (2 * S) == 0 and R // (2 * S) >= 512 and (S < 32 or R // S > 16384):
        S *= 2
    wide = {} if gy.dtype == f32 else {'out_dtype': f32}
    if S == 1:
        return torch.mm(gy.t(), x, **wide)
    return torch.bmm(gy.view(S, R // S, gy.shape[1]).transpose(1, 2), x.view(S, R // S, x.shape[1]), **wide).sum(dim=0)


# ----------------------------------------------------------------------------- fp16 gradients: range scaling
# fp16 has 5 exponent bits: normals from 6.1e-5, nothing below 6e-8.  Under a mean-reduced loss the gradient that reaches a
# transformer block is 1e-6 .. 1e-5 at its largest, and every 16-bit tensor of the backward (the incoming gradient rounded for
# the GEMMs, dL, da, dT1, dU, d delta, dT0) would sit in the subnormals or round to 0.  The backward is linear in its incoming
# gradient, so it runs on s * g with s the power of two that brings max|g| into [2^(t-1), 2^t), and its fp32 results are
# multiplied by 1 / s: exact (a change of exponent), computed on the device from the bits of max|g| (sug_grad_scale16: no
# host read, no synchronisation: capturable), and absent from the fp32 mode.
# t = 4 (max|s g| in [8, 16)).  Headroom above, to fp16's 65504 = 2^16: da = g a <= 16 (softmax weights a <= 1, reached in the
# saturated regime): 2^12; dL = a (g y - g mixed) / sqrt(512) <= 16 * 2 max|y| * 0.044 = 14 for |V + delta| = 10: 2^12; the
# GEMM results dT1, dU, dT0 grow with the weights' row norms: sqrt(512) * |w| * |dL| is estimated at 16 for the default
# initialisation and 640 with fc_gamma[2] multiplied by 1024 (softmax weights up to 1.0), peaks a few times that: 2^4 at the
# least.  The estimate is held by tests/test_gpu_ptran.py at that gain (finite gradients, the same at every loss scale); an
# overflow would put inf into every gradient of the block.  Room below: a gradient 2^-10 of the largest is still a normal
# number (an O(1) probe used to leave 2^-14: the scaling also gains 2^4 there).
_G16_LOG2_TARGET = 4


def _grad_scale16(*gs):
    """(s, 1 / s) as 0-dim fp32 device tensors for up to three contiguous fp32 tensors: s = 2^(t - floor(log2(max|g|)) - 1),
    clamped to 2^+-100 (max|g| = 0: 2^100 * 0 = 0; inf / nan pass through g as they are).  sug_grad_scale16: two kinds of
    launches, no memset (a torch reduction to one element brings one), nothing read by the host."""
    gs = [g if g.is_contiguous() else g.contiguous() for g in gs]
    dev = gs[0].device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    ws = torch.empty(768, dtype=torch.float32, device=dev)
    a = [(_p(g), g.numel()) for g in gs] + [(None, 0)] * (3 - len(gs))
    check(lib().sug_grad_scale16(a[0][0], a[0][1], a[1][0], a[1][1], a[2][0], a[2][1], _G16_LOG2_TARGET, _p(out), _p(ws), _st()),
          'sug_grad_scale16')
    return out[0], out[1]


def _scaled16(g2, s):
    """(s * g2) rounded to fp16 in one pass."""
    return torch.mul(g2, s, out=torch.empty_like(g2, dtype=torch.float16))


class _Linear16(torch.autograd.Function):
    """nn.Linear on [..., K] rows with 16-bit operands (MFMA, fp32 accumulation) and fp32 parameters: the weight's
    16-bit copy comes from the step cache, the result leaves the GEMM as fp32 (`out32`) or stays 16-bit for a
    following 16-bit GEMM, the parameter gradients leave their GEMMs as fp32 (split-K over row chunks).  Written
    out so that no cast kernels surround the GEMMs (an F.linear on cast operands costs ~6 per call)."""

    @staticmethod
    def forward(ctx, x, w, b, lo, out32):
        _need_gpu(x, w)
        x2 = x.reshape(-1, x.shape[-1])
        x16 = x2 if x2.dtype == lo else x2.to(lo)
        w16 = cast_cached(w, lo, detach=True)
        if out32:
            y = torch.mm(x16, w16.t(), out_dtype=torch.float32)
            if b is not None:
                y += b
        elif b is None:
            y = torch.mm(x16, w16.t())
        else:
            y = torch.addmm(cast_cached(b, lo, detach=True), x16, w16.t())
        ctx.save_for_backward(x16, w16)
        ctx.meta = (x.shape, x.dtype, b is not None, lo)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, g):
        x16, w16 = ctx.saved_tensors
        xshape, xdtype, has_b, lo = ctx.meta
        g2 = g.reshape(-1, g.shape[-1])
        # an fp32 gradient rounded to fp16 for GEMMs with fp32 results: on s * g, results * 1 / s (_grad_scale16)
        scaled = lo == torch.float16 and g2.dtype == torch.float32 and xdtype == torch.float32
        if scaled:
            s, inv = _grad_scale16(g2)
            g16 = _scaled16(g2, s)
        else:
            g16 = g2 if g2.dtype == lo else g2.to(lo)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = (torch.mm(g16, w16, out_dtype=torch.float32) if xdtype == torch.float32 else torch.mm(g16, w16)).view(xshape)
        dw = _dweight(g16, x16) if ctx.needs_input_grad[1] else None
        db = colsum(g2) if (has_b and ctx.needs_input_grad[2]) else None
        if scaled:
            torch._foreach_mul_([t for t in (dx, dw) if t is not None], inv)
        return dx, dw, db, None, None


def linear16(x, layer, lo, out32=True):
    return _Linear16.apply(x, layer.weight, layer.bias, lo, out32)


class _LiftProject16(torch.autograd.Function):
    """fc1 and the three projections w_qs / w_ks / w_vs of a TransformerBlock with 16-bit operands and fp32 parameters:
    lifted = fc1(x) stays 16-bit between them (one rounding, no re-casts), and so does its gradient.  That gradient is why the
    four linears share one backward: in fp16 it is only representable scaled (_grad_scale16), and a scale cannot travel
    between autograd nodes; here s * d lifted never leaves the function.  Forward values as four _Linear16 calls."""

    @staticmethod
    def forward(ctx, x, w1, b1, wq, wk, wv, lo):
        _need_gpu(x, w1)
        x2 = x.reshape(-1, x.shape[-1])
        x16 = x2 if x2.dtype == lo else x2.to(lo)
        w16 = cast_cached(w1, lo, detach=True)
        lifted = torch.addmm(cast_cached(b1, lo, detach=True), x16, w16.t())
        wp = [cast_cached(w, lo, detach=True) for w in (wq, wk, wv)]
        ctx.save_for_backward(x16, w16, lifted, *wp)
        ctx.meta = (x.shape, lo)
        return tuple(torch.mm(lifted, w.t(), out_dtype=torch.float32).view(*x.shape[:-1], w.shape[0]) for w in wp)

    @staticmethod
    def backward(ctx, *gs):
        x16, w16, lifted, *wp = ctx.saved_tensors
        xshape, lo = ctx.meta
        gs = [g.reshape(-1, g.shape[-1]).float() for g in gs]
        if lo == torch.float16:
            s, inv = _grad_scale16(*gs)
            g16 = [_scaled16(g, s) for g in gs]
        else:
            g16 = [g.to(lo) for g in gs]
        need = ctx.needs_input_grad
        dwp = [_dweight(g, lifted) if need[3 + i] else None for i, g in enumerate(g16)]
        dx = dw1 = db1 = None
        if need[0] or need[1] or need[2]:
            # s * d lifted, 16-bit: the three GEMMs and their sum as autograd runs them for three separate linears
            dl = torch.mm(g16[0], wp[0])
            dl += torch.mm(g16[1], wp[1])
            dl += torch.mm(g16[2], wp[2])
            if need[1]:
                dw1 = _dweight(dl, x16)
            if need[2]:
                db1 = colsum(dl) if lo == torch.float16 else dl.sum(0, dtype=torch.float32)
            if need[0]:
                dx = torch.mm(dl, w16, out_dtype=torch.float32).view(xshape)
        if lo == torch.float16:
            torch._foreach_mul_([t for t in (dx, dw1, db1, *dwp) if t is not None], inv)
        return dx, dw1, db1, dwp[0], dwp[1], dwp[2], None


def lift_project16(x, fc1, w_qs, w_ks, w_vs, lo):
    """(q, K, V) = (w_qs, w_ks, w_vs)(fc1(x)) on the 16-bit path, fp32 results."""
    return _LiftProject16.apply(x, fc1.weight, fc1.bias, w_qs.weight, w_ks.weight, w_vs.weight, lo)


# ----------------------------------------------------------------------------- Point Transformer attention
# fp16 mode: the forward of a transformer block's vector attention as ONE MFMA kernel (sug_ptran_fused_fwd) instead of pos1 +
# 3 library GEMMs + qk + attn.  Same roundings, another order of the GEMMs' partial sums: outputs within 2e-3 of the composed
# chain's (relative L2 3e-4), and no further from fp64 than 2 x the chain's own error (tests/test_gpu_ptran.py).  Measured at
# config 5's block-1 shape (1 M k-expanded rows; tools/bench_ptran_fused.py, profiles/r06_ptran_fused_ab.txt): without a
# backward to feed 2.56 vs 3.21 ms -- nothing but delta is written --, with the four tensors a backward reads 3.11 vs 3.13 ms,
# and 19.73 vs 19.63 ms for the whole config-5 step as it stood in round 6 (before the range scaling of the fp16 backward,
# which costs both forms the same 1.5 ms: profiles/ptran_fp16_grad_scale_ab.txt): one 130 KB workgroup per CU serialises its
# row passes (L2 gathers of K / V rows) with its MFMA chains, the composition overlaps them across kernels at full occupancy.
# Hence 'auto': the one-kernel form where no backward follows (eval / no_grad forwards), the composition in training.
# SUG_PTRAN_FUSED=1 / 0 forces one form.
PTRAN_FUSED = {'1': True, '0': False}.get(_os.environ.get('SUG_PTRAN_FUSED', 'auto'), 'auto')


class _PTranAttention(torch.autograd.Function):
    """Vector attention of one TransformerBlock (model/Ptran_transformer.py:39-44) from the projected
    q / K / V rows: pos-encoding MLP on the neighbour offsets, attention MLP on q - k + delta, softmax
    over the k neighbours per channel, weighted sum of v + delta.  The three 512 x 512 linears on the
    k-expanded rows are library GEMMs in `dtype` (fp32 = the reference's arithmetic; fp16 = MFMA with
    fp32 accumulation, BASELINE config 5); everything between them is sug_ptran_* (one pass each).
    The backward is written out by hand: nothing but the GEMM operands T0, delta, U, T1, L is saved, the
    two gradients of delta are summed inside sug_ptran_qk_bwd, dK / dV are gathered over reverse
    neighbour lists (deterministic, no atomics)."""

    @staticmethod
    def forward(ctx, xyz, nbr, q, kf, vf, w1, b1, w2, b2, wg1, bg1, wg2, bg2, dtype):
        _need_gpu(xyz, nbr, q, kf, vf)
        B, n, k = nbr.shape
        d = q.shape[-1]
        dev = q.device
        lo = torch.float32 if dtype is None else dtype
        code = 0 if lo == torch.float32 else 1
        if lo not in (torch.float32, torch.float16):
            raise RuntimeError('ptran_attention: fp32 or fp16 (got %s)' % lo)
        R = B * n * k
        xyz, nbr = xyz.detach().contiguous(), _i32(nbr).contiguous()
        q, kf, vf = q.contiguous(), kf.contiguous(), vf.contiguous()
        w1c, b1c = w1.detach().contiguous(), b1.detach().contiguous()
        wl = [cast_cached(t, lo, detach=True) for t in (w2, b2, wg1, bg1, wg2, bg2)]
        L_ = lib()
        scale = 1.0 / (d ** 0.5)
        need = any(ctx.needs_input_grad[i] for i in range(2, 13))
        if (PTRAN_FUSED is True or (PTRAN_FUSED == 'auto' and not need)) and code == 1 and L_.sug_ptran_fused_supported(B, n, k, d):
            # the whole fp16 forward as ONE kernel on the matrix cores (csrc/ptran_fused.hip): no library GEMM, no k-expanded
            # tensor read back; T0 / U / T1 / logits are written (once) only when a backward will read them
            delta = torch.empty(R, d, dtype=lo, device=dev)
            T0, U, T1, Lg = ((torch.empty(R, d, dtype=lo, device=dev) for _ in range(4)) if need else (None,) * 4)
            mixed = torch.empty(B, n, d, dtype=torch.float32, device=dev)
            mx, sm = torch.empty_like(mixed), torch.empty_like(mixed)
            shp = {'B': B, 'N': n, 'k': k, 'd': d, 'e': 2}
            check(_timed('ptran_fused_fwd_n%d' % n, shp, lambda: L_.sug_ptran_fused_fwd(
                _p(xyz), _p(nbr), _p(q), _p(kf), _p(vf), _p(w1c), _p(b1c), _p(wl[0]), _p(wl[1]), _p(wl[2]), _p(wl[3]), _p(wl[4]),
                _p(wl[5]), B, n, k, d, scale, 1 if need else 0, _p(T0), _p(delta), _p(U), _p(T1), _p(Lg), _p(mixed), _p(mx), _p(sm),
                _st())), 'sug_ptran_fused_fwd')
            if need:
                ctx.save_for_backward(xyz, nbr, vf, w1c, b1c, wl[0], wl[2], wl[4], T0, delta, U, T1, Lg, mx, sm, mixed)
            ctx.meta = (B, n, k, d, code, scale)
            return mixed
        T0 = torch.empty(R, d, dtype=lo, device=dev)
        check(L_.sug_ptran_pos1_fwd(_p(xyz), _p(nbr), _p(w1c), _p(b1c), B, n, k, d, code, _p(T0), _st()), 'sug_ptran_pos1_fwd')
        delta = torch.addmm(wl[1], T0, wl[0].t())
        U = torch.empty(R, d, dtype=lo, device=dev)
        shp = {'B': B, 'N': n, 'k': k, 'd': d, 'e': 4 if code == 0 else 2}
        check(_timed('ptran_qk_fwd_n%d' % n, shp, lambda: L_.sug_ptran_qk_fwd(_p(q), _p(kf), _p(delta), _p(nbr), B, n, k, d, code, _p(U), _st())),
              'sug_ptran_qk_fwd')
        T1 = torch._addmm_activation(wl[3], U, wl[2].t())          # bias + ReLU in the library GEMM's epilogue
        Lg = torch.addmm(wl[5], T1, wl[4].t())
        mixed = torch.empty(B, n, d, dtype=torch.float32, device=dev)
        mx, sm = torch.empty_like(mixed), torch.empty_like(mixed)
        check(_timed('ptran_attn_fwd_n%d' % n, shp, lambda: L_.sug_ptran_attn_fwd(_p(Lg), _p(delta), _p(vf), _p(nbr), B, n, k, d, code, scale,
                                                                          _p(mixed), _p(mx), _p(sm), _st())), 'sug_ptran_attn_fwd')
        ctx.save_for_backward(xyz, nbr, vf, w1c, b1c, wl[0], wl[2], wl[4], T0, delta, U, T1, Lg, mx, sm, mixed)
        ctx.meta = (B, n, k, d, code, scale)
        return mixed

    @staticmethod
    def backward(ctx, g):
        xyz, nbr, vf, w1c, b1c, w2l, wg1l, wg2l, T0, delta, U, T1, Lg, mx, sm, mixed = ctx.saved_tensors
        B, n, k, d, code, scale = ctx.meta
        dev, lo = g.device, T0.dtype
        L_ = lib()
        g = g.contiguous().float()
        if code == 1:           # the fp16 chain runs on s * g (_grad_scale16); its fp32 results are multiplied by 1 / s below
            s, inv = _grad_scale16(g)
            g = g * s
        off, ent = knn_reverse(nbr)
        dL, da = torch.empty_like(Lg), torch.empty_like(Lg)
        dv = torch.empty(B, n, d, dtype=torch.float32, device=dev)
        f32 = torch.float32
        # bias gradients = column sums of the k-expanded gradients, produced by the kernels that write them
        R = B * n * k
        cws = torch.empty(L_.sug_ptran_colsum_workspace(R), dtype=f32, device=dev)
        dbg2, dbg1, db2 = (torch.empty(d, dtype=f32, device=dev) for _ in range(3))
        shp = {'B': B, 'N': n, 'k': k, 'd': d, 'e': 4 if code == 0 else 2}
        check(_timed('ptran_attn_bwd_n%d' % n, shp, lambda: L_.sug_ptran_attn_bwd(_p(g), _p(mixed), _p(Lg), _p(delta), _p(vf), _p(nbr), _p(mx),
                                                                          _p(sm), _p(off), _p(ent), B, n, k, d, code, scale, _p(dL),
                                                                          _p(da), _p(dv), _p(dbg2), _p(cws), _st())),
              'sug_ptran_attn_bwd')

        dwg2 = _dweight(dL, T1)
        dT1 = dL @ wg2l
        check(L_.sug_ptran_relu_bwd_db(_p(dT1), _p(T1), R, d, code, _p(dbg1), _p(cws), _st()), 'sug_ptran_relu_bwd_db')
        dwg1 = _dweight(dT1, U)
        dU = dT1 @ wg1l
        dq, dk = torch.empty_like(dv), torch.empty_like(dv)
        check(_timed('ptran_qk_bwd_n%d' % n, shp, lambda: L_.sug_ptran_qk_bwd(_p(dU), _p(da), _p(off), _p(ent), B, n, k, d, code, _p(dq), _p(dk),
                                                                      _p(db2), _p(cws), _st())), 'sug_ptran_qk_bwd')
        ddelta = da                                            # = dU + da
        dw2 = _dweight(ddelta, T0)
        dT0 = ddelta @ w2l
        dw1 = torch.empty(d, 3, dtype=f32, device=dev)
        db1 = torch.empty(d, dtype=f32, device=dev)
        ws = torch.empty(1024 * 4 * d, dtype=f32, device=dev)
        check(L_.sug_ptran_pos1_bwd(_p(dT0), _p(xyz), _p(nbr), _p(w1c), _p(b1c), B, n, k, d, code, _p(dw1), _p(db1), _p(ws),
                                    _st()), 'sug_ptran_pos1_bwd')
        if code == 1:
            torch._foreach_mul_([dq, dk, dv, dw1, db1, dw2, db2, dwg1, dbg1, dwg2, dbg2], inv)
        return None, None, dq, dk, dv, dw1, db1, dw2, db2, dwg1, dbg1, dwg2, dbg2, None


def ptran_attention(xyz, nbr, q, kf, vf, fc_delta, fc_gamma, dtype=None):
    """xyz [B,n,3], nbr [B,n,k], q / kf / vf [B,n,512] (w_qs / w_ks / w_vs of the lifted features),
    fc_delta = Sequential(Linear(3,512), ReLU, Linear(512,512)), fc_gamma likewise (512,512) -> [B,n,512]."""
    return _PTranAttention.apply(xyz, nbr, q, kf, vf, fc_delta[0].weight, fc_delta[0].bias, fc_delta[2].weight,
                                 fc_delta[2].bias, fc_gamma[0].weight, fc_gamma[0].bias, fc_gamma[2].weight,
                                 fc_gamma[2].bias, dtype)


# ----------------------------------------------------------------------------- channel attention (CALayer)
CALAYER_FUSED = _os.environ.get('SUG_CALAYER_FUSED', '1') != '0'    # A/B knob: 0 = library GEMMs + relu + gate_bn per layer
GATE_BN_MULTI = _os.environ.get('SUG_GATE_BN_MULTI', '1') != '0'    # A/B knob: 0 = one sug_gate_bn_fwd / _bwd launch per layer


def calayer_supported(layers, x):
    """Can the CALayer modules `layers` (1 or 2: attention_s [, attention_t]) run through sug_calayer_* on x [len(layers)*M, C]?"""
    if not (CALAYER_FUSED and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and CTX.bn_groups == 1):
        return False
    if x.shape[0] % len(layers):
        return False
    M, C = x.shape[0] // len(layers), x.shape[1]
    for m in layers:
        c0, c2, bn = m.conv_du[0], m.conv_du[2], m.bn
        if c0.weight.shape[1] != C or c2.weight.shape[0] != C or c0.bias is None or c2.bias is None or not bn.affine \
                or not (bn.training or bn.track_running_stats) or bn.momentum is None or not bn.track_running_stats:
            return False
        if any(mm.training != layers[0].training for mm in (m, bn)):
            return False
    return bool(lib().sug_calayer_supported(len(layers), M, C, layers[0].conv_du[0].weight.shape[0]))


class _CALayers(torch.autograd.Function):
    """BatchNorm1d(v * sigmoid(z) + v), z = W2 . relu(W0 . v + b0) + b2 (CALayer, model/Model.py:28-34) for one or two
    attention layers on the row blocks of x [layers*M, C]: sug_calayer_fwd / _bwd + sug_gate_bn_fwd / _bwd.
    params per layer: W0 [Hd,C], b0, W2 [C,Hd], b2, gamma, beta, running_mean, running_var."""

    @staticmethod
    def forward(ctx, x, nl, training, eps, momentum, *params):
        _need_gpu(x)
        x = x if (x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0) else x.contiguous()
        M, C = x.shape[0] // nl, x.shape[1]
        P = [params[8 * a:8 * a + 8] for a in range(nl)]
        W0 = [p[0].detach().reshape(p[0].shape[0], -1).contiguous() for p in P]
        W2 = [p[2].detach().reshape(p[2].shape[0], -1).contiguous() for p in P]
        b0, b2 = [p[1].detach().contiguous() for p in P], [p[3].detach().contiguous() for p in P]
        gam, bet = [p[4].detach().contiguous() for p in P], [p[5].detach().contiguous() for p in P]
        Hd = W0[0].shape[0]
        dev = x.device
        L = lib()
        hp = torch.empty(nl, C // 512, M, Hd, dtype=torch.float32, device=dev)
        h = torch.empty(nl, M, Hd, dtype=torch.float32, device=dev)
        z = torch.empty(nl * M, C, dtype=torch.float32, device=dev)
        check(L.sug_calayer_fwd(nl, _p(x), x.stride(0), M, C, Hd, _ptrs(W0), _ptrs(b0), _ptrs(W2), _ptrs(b2), _p(hp), _p(h), _p(z),
                                _st()), 'sug_calayer_fwd')
        out = torch.empty(nl * M, C, dtype=torch.float32, device=dev)
        stat = torch.empty(nl, 2, C, dtype=torch.float32, device=dev)
        xc = x if x.stride(0) == C else x.contiguous()            # (sug_gate_bn_* take dense rows)
        multi = GATE_BN_MULTI and 1 < nl <= 4
        if multi:                         # both layers' gate + BatchNorm in one launch
            check(L.sug_gate_bn_fwd_multi(nl, _p(xc), _p(z), M, C, _ptrs(gam), _ptrs(bet), _ptrs([p[6] for p in P]),
                                          _ptrs([p[7] for p in P]), 1 if training else 0, float(eps), float(momentum), _p(out),
                                          _p(stat), _st()), 'sug_gate_bn_fwd_multi')
        for a in range(0 if multi else nl):
            check(L.sug_gate_bn_fwd(_p(xc[a * M:]), _p(z[a * M:]), M, C, _p(gam[a]), _p(bet[a]), _p(P[a][6]), _p(P[a][7]),
                                    1 if training else 0, float(eps), float(momentum), _p(out[a * M:]), _p(stat[a]), _st()),
                  'sug_gate_bn_fwd')
        ctx.save_for_backward(xc, h, z, stat, *W0, *W2, *gam)
        ctx.meta = (nl, M, C, Hd, bool(training), multi)
        return out

    @staticmethod
    def backward(ctx, g):
        nl, M, C, Hd, training, multi = ctx.meta
        sv = ctx.saved_tensors
        x, h, z, stat = sv[:4]
        W0, W2, gam = sv[4:4 + nl], sv[4 + nl:4 + 2 * nl], sv[4 + 2 * nl:4 + 3 * nl]
        dev = x.device
        L = lib()
        g = g.contiguous()
        dxg, dz = torch.empty_like(x), torch.empty_like(x)
        dgb = torch.empty(nl, 2, C, dtype=torch.float32, device=dev)
        if multi:
            check(L.sug_gate_bn_bwd_multi(nl, _p(g), _p(x), _p(z), M, C, _ptrs(gam), _p(stat), 1 if training else 0, _p(dxg), _p(dz),
                                          _p(dgb), _st()), 'sug_gate_bn_bwd_multi')
        for a in range(0 if multi else nl):
            check(L.sug_gate_bn_bwd(_p(g[a * M:]), _p(x[a * M:]), _p(z[a * M:]), M, C, _p(gam[a]), _p(stat[a]), 1 if training else 0,
                                    _p(dxg[a * M:]), _p(dz[a * M:]), _p(dgb[a, 0]), _p(dgb[a, 1]), _st()), 'sug_gate_bn_bwd')
        f32 = torch.float32
        dW0 = [torch.empty(Hd, C, dtype=f32, device=dev) for _ in range(nl)]
        dW2 = [torch.empty(C, Hd, dtype=f32, device=dev) for _ in range(nl)]
        db0 = [torch.empty(Hd, dtype=f32, device=dev) for _ in range(nl)]
        db2 = [torch.empty(C, dtype=f32, device=dev) for _ in range(nl)]
        dhp = torch.empty(nl, C // 32, M, Hd, dtype=f32, device=dev)
        dh = torch.empty(nl, M, Hd, dtype=f32, device=dev)
        dx = torch.empty(nl * M, C, dtype=f32, device=dev)
        check(L.sug_calayer_bwd(nl, _p(x), x.stride(0), M, C, Hd, _ptrs(W0), _ptrs(W2), _p(h), _p(dz), _p(dxg), _ptrs(dW0), _ptrs(db0),
                                _ptrs(dW2), _ptrs(db2), _p(dhp), _p(dh), _p(dx), C, _st()), 'sug_calayer_bwd')
        grads = []
        for a in range(nl):
            grads += [dW0[a].view(Hd, C, 1, 1), db0[a], dW2[a].view(C, Hd, 1, 1), db2[a], dgb[a, 0], dgb[a, 1], None, None]
        return (dx, None, None, None, None) + tuple(grads)


def calayers(layers, x):
    """[attention(x rows of its block) for attention in layers] as one [len(layers)*M, C] tensor (rows of layer 0 first)."""
    params = []
    for m in layers:
        _count_bn_call(m.bn)
        c0, c2 = m.conv_du[0], m.conv_du[2]
        params += [c0.weight, c0.bias, c2.weight, c2.bias, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var]
    bn = layers[0].bn
    return _CALayers.apply(x, len(layers), bn.training, bn.eps, bn.momentum, *params)


# ----------------------------------------------------------------------------- clouds as rows
_rows_cache = [None, None, None]           # weakref to the [B,3,N,1] input, its version, the [B,N,3] rows


def clear_rows_cache():
    """Drop the cached rows of the last batch (SUGStep does after every step: the rows of a captured step live in the
    graph's memory pool and must not be pinned by a module global)."""
    _rows_cache[0] = _rows_cache[1] = _rows_cache[2] = None


def cloud_rows(x):
    """x [B,3(+),N,1] (the reference's cloud layout) -> [B,N,3(+)] contiguous rows.  The semantic and the node pass of a step
    (and the Chamfer weights) transpose the same batch: the last result is kept, keyed on the tensor OBJECT (weak
    reference) and its version, so the copy is made once per batch.
    CONTRACT of the key: a write into `x` that does not bump `x._version` -- `x.data` arithmetic, a numpy view of the same
    memory, a raw-pointer kernel -- is NOT seen; whoever refills a batch buffer that way calls clear_rows_cache() (or uses
    copy_ / an in-place torch op, which bump the version).  SUGStep clears the cache at the end of every step."""
    import weakref
    ref, ver, rows = _rows_cache
    if ref is not None and ref() is x and ver == x._version and not x.requires_grad:
        return rows
    rows = x.squeeze(-1).transpose(1, 2).contiguous()
    if not x.requires_grad and not torch.is_inference_mode_enabled():
        _rows_cache[0], _rows_cache[1], _rows_cache[2] = weakref.ref(x), x._version, rows
    return rows


# ----------------------------------------------------------------------------- scalar tail of a step
class _CEPair(torch.autograd.Function):
    """w * (CE(logits1[:M], label) + CE(logits2[:M], label)) of both classifier heads on the SOURCE rows of the paired
    logits in one launch (sug_ce_pair_fwd); the backward writes the whole pair's gradient (zeros in the target rows)."""

    @staticmethod
    def forward(ctx, y1, y2, label, w, ignore_index=-100):
        _need_gpu(y1, y2, label)
        M, C = label.shape[0], y1.shape[1]
        a = y1 if y1.stride(1) == 1 else y1.contiguous()
        b = y2 if (y2.stride(1) == 1 and y2.stride(0) == a.stride(0)) else y2.contiguous()
        if b.stride(0) != a.stride(0):
            a, b = a.contiguous(), b.contiguous()
        lab = label.reshape(-1).long().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=y1.device)
        lse = torch.empty(2 * M + 1, dtype=torch.float32, device=y1.device)     # + the number of counting rows
        check(lib().sug_ce_pair_fwd(_p(a), _p(b), a.stride(0), _p(lab), M, C, float(w), int(ignore_index), _p(loss), _p(lse), _st()),
              'sug_ce_pair_fwd')
        ctx.save_for_backward(a, b, lab, lse)
        ctx.meta = (M, y1.shape[0], C, float(w), int(ignore_index))
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b, lab, lse = ctx.saved_tensors
        M, Mtot, C, w, ign = ctx.meta
        gs = g.detach().to(dtype=torch.float32).reshape(1)
        d = torch.empty(2, Mtot, C, dtype=torch.float32, device=a.device)
        check(lib().sug_ce_pair_bwd(_p(a), _p(b), a.stride(0), _p(lab), M, Mtot, C, w, ign, _p(gs), _p(lse), _p(d[0]), _p(d[1]),
                                    _st()), 'sug_ce_pair_bwd')
        return d[0], d[1], None, None, None


CE_PAIR_MAX_ROWS, CE_PAIR_MAX_CLASSES = _H['SUG_CE_PAIR_MAX_ROWS'], _H['SUG_CE_PAIR_MAX_CLASSES']


def ce_pair_supported(y1, y2, label):
    return y1.is_cuda and y1.dtype == torch.float32 and y1.dim() == 2 and y1.shape == y2.shape and y1.shape[1] <= CE_PAIR_MAX_CLASSES \
        and 2 * label.shape[0] <= CE_PAIR_MAX_ROWS and label.shape[0] <= y1.shape[0]


def ce_pair(y1, y2, label, w, ignore_index=-100):
    """y1, y2 [Mtot >= M, C] logits of the two heads (the first M rows are scored), label [M] -> 0-d loss.
    nn.CrossEntropyLoss label semantics: rows labelled `ignore_index` are skipped (and left out of the mean); any other
    label outside [0, C) -- torch raises there -- turns the loss into NaN."""
    return _CEPair.apply(y1, y2, label, w, ignore_index)


CE_MAX_ROWS, CE_MAX_CLASSES = _H['SUG_CE_MAX_ROWS'], _H['SUG_CE_MAX_CLASSES']


class _CE(torch.autograd.Function):
    """nn.CrossEntropyLoss(reduction='mean', ignore_index, label_smoothing) of ONE head in one launch each way
    (sug_ce_fwd / sug_ce_bwd); the forward's launch also adds (loss * M, M) to the caller's `totals`."""

    @staticmethod
    def forward(ctx, y, label, ignore_index, label_smoothing, totals):
        _need_gpu(y, label, totals)
        if y.dim() != 2 or y.dtype != torch.float32 or label.numel() != y.shape[0]:
            raise RuntimeError('ops.ce: fp32 logits [M, C] and M labels (got %s %s, %d labels)' % (tuple(y.shape), y.dtype, label.numel()))
        if totals is not None and (totals.dtype != torch.float64 or totals.numel() != 2 or not totals.is_contiguous()):
            raise RuntimeError('ops.ce: totals is a contiguous float64 tensor of 2 elements')
        M, C = y.shape
        a = y if (y.stride(1) == 1 and y.stride(0) >= C) else y.contiguous()
        lab = label.reshape(-1).long().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=y.device)
        lse = torch.empty(M + 1, dtype=torch.float32, device=y.device)          # + the number of counting rows
        check(lib().sug_ce_fwd(_p(a), a.stride(0), _p(lab), M, C, int(ignore_index), float(label_smoothing), _p(loss), _p(lse),
                               _p(totals), _st()), 'sug_ce_fwd')
        ctx.save_for_backward(a, lab, lse)
        ctx.meta = (M, C, int(ignore_index), float(label_smoothing))
        return loss

    @staticmethod
    def backward(ctx, g):
        a, lab, lse = ctx.saved_tensors
        M, C, ign, eps = ctx.meta
        gs = g.detach().to(dtype=torch.float32).reshape(1)
        d = torch.empty(M, C, dtype=torch.float32, device=a.device)
        check(lib().sug_ce_bwd(_p(a), a.stride(0), _p(lab), M, C, ign, eps, _p(gs), _p(lse), _p(d), _st()), 'sug_ce_bwd')
        return d, None, None, None, None


def ce_supported(y, label):
    return y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and 1 <= y.shape[0] <= CE_MAX_ROWS \
        and 2 <= y.shape[1] <= CE_MAX_CLASSES and label.numel() == y.shape[0]


def ce(logits, label, ignore_index=-100, label_smoothing=0.0, totals=None):
    """logits [M, C] fp32 (any row stride), label [M] -> 0-d loss = nn.CrossEntropyLoss(ignore_index=..., label_smoothing=...)
    with ce_pair's label semantics (ignore_index rows skipped, any other label outside [0, C) -> NaN).  totals: None or a
    device float64 [2] that the same launch advances by (loss * M, M) -- the epoch's books of train_source.py:130-131.
    1 <= M <= 1024, 2 <= C <= 64 (the library refuses anything else)."""
    return _CE.apply(logits, label, ignore_index, label_smoothing, totals)


class _LossCombine(torch.autograd.Function):
    """(loss_cls + wg*v_geo + ws*(v_sem1 + v_sem2), wg*v_geo, ws*(v_sem1 + v_sem2)) in one launch each way; the two parts
    are returned for reporting only (non-differentiable)."""

    @staticmethod
    def forward(ctx, loss_cls, v0, v1, v2, wg, ws):
        out = torch.empty(3, dtype=torch.float32, device=loss_cls.device)
        f = lambda t: None if t is None else t.detach().float()
        lc, a, b, c = f(loss_cls), f(v0), f(v1), f(v2)
        check(lib().sug_loss_combine_fwd(_p(lc), _p(a), _p(b), _p(c), float(wg), float(ws), _p(out), _st()), 'sug_loss_combine_fwd')
        ctx.meta = (float(wg), float(ws), v0 is not None, v1 is not None, v2 is not None)
        tot, geo, sem = out[0], out[1], out[2]
        ctx.mark_non_differentiable(geo, sem)
        ctx.set_materialize_grads(False)          # no zero-filled scalars for the two reporting outputs (a launch each)
        return tot, geo, sem

    @staticmethod
    def backward(ctx, g, _g1, _g2):
        wg, ws, h0, h1, h2 = ctx.meta
        if g is None:
            return None, None, None, None, None, None
        o = torch.empty(4, dtype=torch.float32, device=g.device)
        gs = g.detach().to(dtype=torch.float32).reshape(1)
        check(lib().sug_loss_combine_bwd(_p(gs), wg, ws, _p(o), _st()), 'sug_loss_combine_bwd')
        return o[0], (o[1] if h0 else None), (o[2] if h1 else None), (o[3] if h2 else None), None, None


def loss_combine(loss_cls, v_geo, v_sem1, v_sem2, wg, ws):
    return _LossCombine.apply(loss_cls, v_geo, v_sem1, v_sem2, wg, ws)


MCD_MAX_ROWS, MCD_MAX_CLASSES = _H['SUG_MCD_MAX_ROWS'], _H['SUG_CE_MAX_CLASSES']


class _MCDLoss(torch.autograd.Function):
    """The phase-1 loss of the two-phase UDA step in one launch each way (sug_mcd_loss_fwd / sug_mcd_loss_bwd); the forward's
    launch also advances the caller's `totals`.  yt1 is None: ys1, ys2 are the PAIRED logits [Ms + Mt, C], source rows first
    (Ms = the number of labels), and the backward writes the pair's dense gradient."""

    @staticmethod
    def forward(ctx, ys1, ys2, yt1, yt2, label, label_t, a_s, a_t, r_s, totals):
        _need_gpu(ys1, ys2, yt1, yt2, label, label_t, totals)
        paired = yt1 is None
        Ms, C = label.numel(), ys1.shape[1]
        Mt = ys1.shape[0] - Ms if paired else yt1.shape[0]
        ts = [ys1, ys2] if paired else [ys1, ys2, yt1, yt2]
        if any(t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] != C for t in ts) or ys1.shape != ys2.shape or \
                (not paired and (yt1.shape != yt2.shape or ys1.shape[0] != Ms)) or Mt < 1:
            raise RuntimeError('ops.mcd_loss: fp32 logits [Ms, C] x 2 and [Mt, C] x 2 (or two paired [Ms + Mt, C]) and Ms labels '
                               '(got %s, %d labels)' % ([tuple(t.shape) for t in ts], Ms))
        if a_t != 0 and (label_t is None or label_t.numel() != Mt):
            raise RuntimeError('ops.mcd_loss: a_t != 0 needs Mt = %d target labels' % Mt)
        if totals is not None and (totals.dtype != torch.float64 or totals.numel() != 4 or not totals.is_contiguous()):
            raise RuntimeError('ops.mcd_loss: totals is a contiguous float64 tensor of 4 elements')
        ld = ts[0].stride(0)
        if any(t.stride(1) != 1 or t.stride(0) != ld for t in ts) or ld < C:      # one leading dimension for the four blocks
            ts = [t.contiguous() for t in ts]
            ld = C
        if paired:
            ts = [ts[0], ts[1], ts[0][Ms:], ts[1][Ms:]]
        lab = label.reshape(-1).long().contiguous()
        lab_t = label_t.reshape(-1).long().contiguous() if (a_t != 0 and label_t is not None) else None
        out = torch.empty(4, dtype=torch.float32, device=ys1.device)
        lse = torch.empty(2 * Ms + 2 * Mt, dtype=torch.float32, device=ys1.device)
        check(lib().sug_mcd_loss_fwd(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), ld, _p(lab), _p(lab_t), Ms, Mt, C, float(a_s),
                                     float(a_t), float(r_s), _p(out), _p(lse), _p(totals), _st()), 'sug_mcd_loss_fwd')
        ctx.save_for_backward(lab, lse, *((lab_t,) if lab_t is not None else ()), *ts)
        ctx.meta = (Ms, Mt, C, ld, float(a_s), float(a_t), paired, lab_t is not None)
        loss, ls, adv, lt = out[0], out[1], out[2], out[3]
        ctx.mark_non_differentiable(ls, adv, lt)
        ctx.set_materialize_grads(False)          # no zero-filled scalars for the three reporting outputs (a launch each)
        return loss, ls, adv, lt

    @staticmethod
    def backward(ctx, g, _g1, _g2, _g3):
        Ms, Mt, C, ld, a_s, a_t, paired, has_t = ctx.meta
        if g is None:
            return (None,) * 10
        sv = ctx.saved_tensors
        lab, lse = sv[0], sv[1]
        lab_t = sv[2] if has_t else None
        ts = sv[3 if has_t else 2:]
        gs = g.detach().to(dtype=torch.float32).reshape(1)
        d = torch.empty(2, Ms + Mt, C, dtype=torch.float32, device=lse.device)
        check(lib().sug_mcd_loss_bwd(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), ld, _p(lab), _p(lab_t), Ms, Mt, C, a_s, a_t, _p(gs),
                                     _p(lse), _p(d[0]), _p(d[1]), _p(d[0, Ms:]), _p(d[1, Ms:]), _st()), 'sug_mcd_loss_bwd')
        if paired:
            return (d[0], d[1]) + (None,) * 8
        return (d[0, :Ms], d[1, :Ms], d[0, Ms:], d[1, Ms:]) + (None,) * 6


def mcd_loss_supported(ys1, ys2, yt1=None, yt2=None, label=None, a_t=0.0):
    """Can sug_mcd_loss_* take these logits?  (fp32, C <= 64, at most 1024 rows per domain; the target cross entropy is taken
    against the SOURCE labels by its caller, so a_t != 0 needs Ms == Mt.)  False is not an error: the caller composes the ops."""
    ts = [t for t in (ys1, ys2, yt1, yt2) if t is not None]
    if len(ts) not in (2, 4) or any(not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 for t in ts):
        return False
    C = ys1.shape[1]
    if any(t.shape[1] != C for t in ts) or not 2 <= C <= MCD_MAX_CLASSES or ys1.shape != ys2.shape:
        return False
    if yt1 is None:
        if label is None:
            return False
        Ms, Mt = label.numel(), ys1.shape[0] - label.numel()
    else:
        Ms, Mt = ys1.shape[0], yt1.shape[0]
        if yt1.shape != yt2.shape or (label is not None and label.numel() != Ms):
            return False
    return 1 <= Ms <= MCD_MAX_ROWS and 1 <= Mt <= MCD_MAX_ROWS and (a_t == 0 or Ms == Mt)


def mcd_loss(ys1, ys2, yt1, yt2, label, label_t=None, a_s=1.0, a_t=0.0, r_s=1.0, totals=None):
    """a_s*(CE(ys1) + CE(ys2)) + a_t*(CE(yt1, label_t) + CE(yt2, label_t)) - mean|softmax(yt1) - softmax(yt2)| in one launch each
    way -> (loss, r_s*CEs, -D, a_t*CEt), 0-d; only `loss` is differentiable, the others are the values the trainers report.
    yt1 = yt2 = None: ys1, ys2 are the paired [Ms + Mt, C] logits of Net_MDA.forward_pair(paired_out=True), Ms = len(label).
    A label outside [0, C) -> NaN (no ignore_index).  totals: None or a device float64 [4], advanced by
    (r_s*CEs*Ms, -D*Ms, Ms, Mt) in the same launch -- the books of train_uda.py:180-184."""
    return _MCDLoss.apply(ys1, ys2, yt1, yt2, label, label_t, a_s, a_t, r_s, totals)


def _cls_gamma_ok(gamma):
    return gamma == 0 or 1 <= gamma < float('inf')


class _ClsLoss(torch.autograd.Function):
    """The classification loss of the shipped configurations -- focal / class-weighted loss of both heads on source and target
    rows and the heads' discrepancy -- in one launch each way (sug_cls_loss_fwd / sug_cls_loss_bwd); the forward's launch also
    advances the caller's `totals`.  yt1 is None: ys1, ys2 are the PAIRED logits [Ms + Mt, C], source rows first (Ms = the number
    of labels), and the backward writes the pair's dense gradient."""

    @staticmethod
    def forward(ctx, ys1, ys2, yt1, yt2, label, label_t, alpha, gamma, reduction, ignore_index, a_s, a_t, a_d, r_s, totals):
        _need_gpu(ys1, ys2, yt1, yt2, label, label_t, alpha, totals)
        paired = yt1 is None
        Ms, C = label.numel(), ys1.shape[1]
        Mt = ys1.shape[0] - Ms if paired else yt1.shape[0]
        ts = [ys1, ys2] if paired else [ys1, ys2, yt1, yt2]
        if any(t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] != C for t in ts) or ys1.shape != ys2.shape or \
                (not paired and (yt1.shape != yt2.shape or ys1.shape[0] != Ms)) or Mt < 1:
            raise RuntimeError('ops.cls_loss: fp32 logits [Ms, C] x 2 and [Mt, C] x 2 (or two paired [Ms + Mt, C]) and Ms labels '
                               '(got %s, %d labels)' % ([tuple(t.shape) for t in ts], Ms))
        if a_t != 0 and (label_t is None or label_t.numel() != Mt):
            raise RuntimeError('ops.cls_loss: a_t != 0 needs Mt = %d target labels' % Mt)
        if alpha is not None and (alpha.dim() != 1 or alpha.dtype != torch.float32 or alpha.numel() < C or not alpha.is_contiguous()):
            raise RuntimeError('ops.cls_loss: alpha is a contiguous fp32 tensor of at least C = %d entries' % C)
        if reduction not in ('mean', 'sum'):
            raise RuntimeError("ops.cls_loss: reduction is 'mean' or 'sum' (got %r)" % (reduction,))
        if totals is not None and (totals.dtype != torch.float64 or totals.numel() != 4 or not totals.is_contiguous()):
            raise RuntimeError('ops.cls_loss: totals is a contiguous float64 tensor of 4 elements')
        ld = ts[0].stride(0)
        if any(t.stride(1) != 1 or t.stride(0) != ld for t in ts) or ld < C:      # one leading dimension for the four blocks
            ts = [t.contiguous() for t in ts]
            ld = C
        if paired:
            ts = [ts[0], ts[1], ts[0][Ms:], ts[1][Ms:]]
        lab = label.reshape(-1).long().contiguous()
        lab_t = label_t.reshape(-1).long().contiguous() if (a_t != 0 and label_t is not None) else None
        out = torch.empty(4, dtype=torch.float32, device=ys1.device)
        save = torch.empty(4 * (Ms + Mt) + 2, dtype=torch.float32, device=ys1.device)
        rs = int(reduction == 'sum')
        check(lib().sug_cls_loss_fwd(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), ld, _p(lab), _p(lab_t), Ms, Mt, C, _p(alpha),
                                     float(gamma), rs, int(ignore_index), float(a_s), float(a_t), float(a_d), float(r_s), _p(out),
                                     _p(save), _p(totals), _st()), 'sug_cls_loss_fwd')
        opt = [t for t in (lab_t, alpha) if t is not None]
        ctx.save_for_backward(lab, save, *opt, *ts)
        ctx.meta = (Ms, Mt, C, ld, float(gamma), rs, int(ignore_index), float(a_s), float(a_t), float(a_d), float(r_s), paired,
                    lab_t is not None, alpha is not None)
        loss, ls, adv, lt = out[0], out[1], out[2], out[3]
        ctx.mark_non_differentiable(ls, adv, lt)
        ctx.set_materialize_grads(False)          # no zero-filled scalars for the three reporting outputs (a launch each)
        return loss, ls, adv, lt

    @staticmethod
    def backward(ctx, g, _g1, _g2, _g3):
        Ms, Mt, C, ld, gamma, rs, ign, a_s, a_t, a_d, r_s, paired, has_t, has_a = ctx.meta
        if g is None:
            return (None,) * 15
        sv = list(ctx.saved_tensors)
        lab, save = sv[0], sv[1]
        k = 2
        lab_t = alpha = None
        if has_t:
            lab_t, k = sv[k], k + 1
        if has_a:
            alpha, k = sv[k], k + 1
        ts = sv[k:]
        gs = g.detach().to(dtype=torch.float32).reshape(1)
        d = torch.empty(2, Ms + Mt, C, dtype=torch.float32, device=save.device)
        check(lib().sug_cls_loss_bwd(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), ld, _p(lab), _p(lab_t), Ms, Mt, C, _p(alpha), gamma,
                                     rs, ign, a_s, a_t, a_d, r_s, _p(gs), _p(save), _p(d[0]), _p(d[1]), _p(d[0, Ms:]), _p(d[1, Ms:]),
                                     _st()), 'sug_cls_loss_bwd')
        if paired:
            return (d[0], d[1]) + (None,) * 13
        return (d[0, :Ms], d[1, :Ms], d[0, Ms:], d[1, Ms:]) + (None,) * 11


def cls_loss_supported(ys1, ys2, yt1=None, yt2=None, label=None, label_t=None, alpha=None, gamma=0.0, reduction='mean', a_t=0.0):
    """Can sug_cls_loss_* take this?  (fp32 logits, C <= 64, at most 1024 rows per domain, gamma == 0 or >= 1, alpha a device fp32
    vector of at least C entries, Mt target labels when a_t != 0.)  False is not an error: the caller composes the ops."""
    ts = [t for t in (ys1, ys2, yt1, yt2) if t is not None]
    if len(ts) not in (2, 4) or any(not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 for t in ts):
        return False
    C = ys1.shape[1]
    if any(t.shape[1] != C for t in ts) or not 2 <= C <= MCD_MAX_CLASSES or ys1.shape != ys2.shape:
        return False
    if not _cls_gamma_ok(gamma) or reduction not in ('mean', 'sum'):
        return False
    if alpha is not None and not (alpha.is_cuda and alpha.dtype == torch.float32 and alpha.dim() == 1 and alpha.numel() >= C
                                  and alpha.is_contiguous()):
        return False
    if yt1 is None:
        if label is None:
            return False
        Ms, Mt = label.numel(), ys1.shape[0] - label.numel()
    else:
        Ms, Mt = ys1.shape[0], yt1.shape[0]
        if yt1.shape != yt2.shape or (label is not None and label.numel() != Ms):
            return False
    return 1 <= Ms <= MCD_MAX_ROWS and 1 <= Mt <= MCD_MAX_ROWS and (a_t == 0 or (label_t is not None and label_t.numel() == Mt))


def cls_loss(ys1, ys2, yt1, yt2, label, label_t=None, alpha=None, gamma=0.0, reduction='mean', ignore_index=-100, a_s=1.0, a_t=0.0,
             a_d=0.0, r_s=1.0, totals=None):
    """a_s*Ls + a_t*Lt - a_d*D in one launch each way -> (loss, r_s*Ls, -a_d*D, a_t*Lt), 0-d; only `loss` is differentiable.
    Ls = R(L(ys1, label)) + R(L(ys2, label)), Lt the same on yt1, yt2 against label_t, L = alpha[y] * (1 - p_y)^gamma * (-log p_y)
    (model_utils.focal_loss; alpha None = ones; gamma 0 or >= 1), R = `reduction` over the rows ('mean' or 'sum'),
    D = mean|softmax(yt1) - softmax(yt2)|.  alpha None and gamma 0 is nn.CrossEntropyLoss with its `ignore_index`; otherwise there
    is no ignore label.  Any other label outside [0, C) -> NaN.  yt1 = yt2 = None: ys1, ys2 are the paired [Ms + Mt, C] logits of
    Net_MDA.forward_pair(paired_out=True), Ms = len(label).  a_t = a_d = 0: the target rows are not read and get zero gradient.
    totals: None or a device float64 [4], advanced by (r_s*Ls*Ms, -a_d*D*Ms, Ms, Mt) in the same launch."""
    return _ClsLoss.apply(ys1, ys2, yt1, yt2, label, label_t, alpha, gamma, reduction, ignore_index, a_s, a_t, a_d, r_s, totals)


# ----------------------------------------------------------------------------- evaluation metrics (sug_eval_accumulate)
(EVAL_MAX_ROWS, EVAL_MAX_CLASSES, EVAL_BATCH_COUNT, EVAL_DATA_TOTAL, EVAL_CORRECT_TOTAL, EVAL_ERROR, EVAL_LOSS_TOTAL, EVAL_CLASS_ACC,
 EVAL_CLASS_ROWS, EVAL_CLASS_CORRECT, EVAL_BATCH_ACC) = (_H['SUG_EVAL_' + _n] for _n in (
     'MAX_ROWS', 'MAX_CLASSES', 'BATCH_COUNT', 'DATA_TOTAL', 'CORRECT_TOTAL', 'ERROR', 'LOSS_TOTAL', 'CLASS_ACC', 'CLASS_ROWS',
     'CLASS_CORRECT', 'BATCH_ACC'))


def eval_state(cap, device):
    """A zeroed state block for `cap` batches (SUG_EVAL_STATE_WORDS(cap) int64 / fp64 words, held as int64)."""
    return torch.zeros(EVAL_BATCH_ACC + int(cap), dtype=torch.int64, device=device)


def eval_state_fields(state):
    """The accumulators of a state block (on the host), as a dict of numpy values."""
    s = state.cpu()
    d = s.view(torch.float64).numpy()
    i = s.numpy()
    n = int(i[EVAL_BATCH_COUNT])
    cap = s.numel() - EVAL_BATCH_ACC
    return {'batch_count': n, 'data_total': int(i[EVAL_DATA_TOTAL]), 'correct_total': int(i[EVAL_CORRECT_TOTAL]),
            'error': int(i[EVAL_ERROR]), 'loss_total': float(d[EVAL_LOSS_TOTAL]),
            'class_acc': d[EVAL_CLASS_ACC:EVAL_CLASS_ACC + 2 * EVAL_MAX_CLASSES].reshape(EVAL_MAX_CLASSES, 2).copy(),
            'class_rows': i[EVAL_CLASS_ROWS:EVAL_CLASS_ROWS + EVAL_MAX_CLASSES].copy(),
            'class_correct': i[EVAL_CLASS_CORRECT:EVAL_CLASS_CORRECT + EVAL_MAX_CLASSES].copy(),
            'batch_acc': d[EVAL_BATCH_ACC:EVAL_BATCH_ACC + min(n, cap)].copy()}


def eval_accumulate_supported(logits, label):
    return logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 \
        and 1 <= logits.shape[0] <= EVAL_MAX_ROWS and 1 <= logits.shape[1] <= EVAL_MAX_CLASSES \
        and label.is_cuda and label.dtype == torch.int64 and label.dim() == 1 and label.shape[0] == logits.shape[0]


def eval_accumulate(state, logits1, label, logits2=None, loss=None, ce=None, out=None, pred=None, cls_eval=True):
    """One evaluation batch into `state` (sug_eval_accumulate): output = (logits1 + logits2) / 2 (or logits1), its argmax,
    and either the fused cross entropy `ce` = (reduction 'mean' | 'sum', ignore_index, label_smoothing) or the caller's loss
    scalar `loss`.  out [B, C] / pred [B] int64: optional outputs.  No host synchronisation."""
    _need_gpu(logits1, logits2, label, loss, out, pred, state)
    B, C = logits1.shape
    if logits2 is not None and (logits2.shape != logits1.shape or logits2.stride() != logits1.stride()):
        raise RuntimeError('eval_accumulate: the two heads need the same shape and strides')
    if out is not None and not (out.shape == (B, C) and out.is_contiguous() and out.dtype == torch.float32):
        raise RuntimeError('eval_accumulate: out must be a dense fp32 [B, C] tensor')
    if pred is not None and not (pred.shape == (B,) and pred.is_contiguous() and pred.dtype == torch.int64):
        raise RuntimeError('eval_accumulate: pred must be a dense int64 [B] tensor')
    if label.dtype != torch.int64 or not label.is_contiguous() or label.shape != (B,):
        raise RuntimeError('eval_accumulate: label must be a dense int64 [B] tensor')
    if ce is not None:
        mode, ignore_index, smoothing = {'mean': 1, 'sum': 2}[ce[0]], int(ce[1]), float(ce[2])
        lin = None
    else:
        if loss is None:
            raise RuntimeError('eval_accumulate: give the batch loss or a fused cross entropy')
        mode, ignore_index, smoothing = 0, -100, 0.0
        lin = loss.detach().reshape(1).to(torch.float32)
    cap = state.numel() - EVAL_BATCH_ACC
    check(lib().sug_eval_accumulate(_p(logits1), _p(logits2), logits1.stride(0), _p(label), B, C, _p(lin), mode, ignore_index,
                                    smoothing, _p(out), _p(pred), int(bool(cls_eval)), _p(state), cap, _st()),
          'sug_eval_accumulate')


# ----------------------------------------------------------------------------- dense prediction (csrc/seg.hip)
(POINT_CE_MAX_ROWS, POINT_CE_MAX_CLASSES, POINT_CE_BLOCK_ROWS, POINT_CE_PARTIAL_WORDS) = (_H['SUG_POINT_CE_' + _n] for _n in (
    'MAX_ROWS', 'MAX_CLASSES', 'BLOCK_ROWS', 'PARTIAL_WORDS'))
(SEG_MAX_PARTS, SEG_MAX_CATEGORIES, SEG_MAX_CATEGORY_PARTS, SEG_MAX_CLOUDS, SEG_RECORD_WORDS, SEG_SHAPES, SEG_POINTS, SEG_CORRECT,
 SEG_ERROR, SEG_CAT_IOU, SEG_CAT_SHAPES, SEG_PART_POINTS, SEG_PART_CORRECT, SEG_STATE_WORDS) = (_H['SUG_SEG_' + _n] for _n in (
     'MAX_PARTS', 'MAX_CATEGORIES', 'MAX_CATEGORY_PARTS', 'MAX_CLOUDS', 'RECORD_WORDS', 'SHAPES', 'POINTS', 'CORRECT', 'ERROR',
     'CAT_IOU', 'CAT_SHAPES', 'PART_POINTS', 'PART_CORRECT', 'STATE_WORDS'))


class _PointCE(torch.autograd.Function):
    """F.cross_entropy(logits [M, C], label [M], weight, ignore_index, reduction='mean') over sug_point_ce_fwd (two launches)
    and sug_point_ce_bwd (one); the forward's fold also advances the caller's `totals` and, when asked, writes the arg-max."""

    @staticmethod
    def forward(ctx, y, label, weight, ignore_index, totals, want_pred):
        _need_gpu(y, label, weight, totals)
        if y.dim() != 2 or y.dtype != torch.float32 or label.numel() != y.shape[0]:
            raise RuntimeError('ops.point_ce: fp32 logits [..., C] and one label per row (got %s %s, %d labels)'
                               % (tuple(y.shape), y.dtype, label.numel()))
        M, C = y.shape
        if weight is not None and (weight.dtype != torch.float32 or weight.numel() != C):
            raise RuntimeError('ops.point_ce: weight is an fp32 tensor of C = %d elements' % C)
        if totals is not None and (totals.dtype != torch.float64 or totals.numel() != 2 or not totals.is_contiguous()):
            raise RuntimeError('ops.point_ce: totals is a contiguous float64 tensor of 2 elements')
        a = y if (y.stride(1) == 1 and y.stride(0) >= C) else y.contiguous()
        lab = label.reshape(-1).long().contiguous()
        w = None if weight is None else weight.detach().reshape(-1).contiguous()
        words = -(-M // POINT_CE_BLOCK_ROWS) * POINT_CE_PARTIAL_WORDS             # sug_point_ce_workspace(M), without the call
        loss = torch.empty((), dtype=torch.float32, device=y.device)
        lse = torch.empty(2 * M + 1, dtype=torch.float32, device=y.device)      # maxima | log-sums | the denominator
        pred = torch.empty(M, dtype=torch.int32, device=y.device) if want_pred else None
        ws = torch.empty(words, dtype=torch.float64, device=y.device)
        check(lib().sug_point_ce_fwd(_p(a), a.stride(0), _p(lab), M, C, int(ignore_index), _p(w), _p(loss), _p(lse), _p(pred),
                                     _p(ws), _p(totals), _st()), 'sug_point_ce_fwd')
        ctx.save_for_backward(a, lab, lse, w)
        ctx.meta = (M, C, int(ignore_index))
        if want_pred:
            ctx.mark_non_differentiable(pred)
            return loss, pred
        return loss, None

    @staticmethod
    def backward(ctx, g, _gpred=None):
        a, lab, lse, w = ctx.saved_tensors
        M, C, ign = ctx.meta
        gs = g.detach().to(dtype=torch.float32).reshape(1)
        d = torch.empty(M, C, dtype=torch.float32, device=a.device)
        check(lib().sug_point_ce_bwd(_p(a), a.stride(0), _p(lab), M, C, ign, _p(w), _p(gs), _p(lse), _p(d), _st()),
              'sug_point_ce_bwd')
        return d, None, None, None, None, None


def point_ce_supported(logits, label):
    """What point_ce takes: fp32 logits [..., C] on the HIP device with 2 <= C <= 64 and 1 <= rows <= 2^22, one label per row."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() >= 1):
        return False
    C = logits.shape[-1]
    if not 2 <= C <= POINT_CE_MAX_CLASSES:
        return False
    M = logits.numel() // C
    return 1 <= M <= POINT_CE_MAX_ROWS and label.is_cuda and label.numel() == M and not label.is_floating_point()


def point_ce(logits, label, weight=None, ignore_index=-100, totals=None, want_pred=False):
    """logits [..., C] fp32 (the leading dimensions are flattened to rows), label: one integer per row -> the 0-d loss
    F.cross_entropy(rows, label, weight=weight, ignore_index=ignore_index) -- the mean divides by the sum of weight[label]
    over the counting rows -- and, with want_pred, (loss, pred): the rows' arg-max (int32, lowest index on ties, ignored rows
    included) in the leading dimensions' shape.  Labels as ops.ce takes them (ignore_index rows skipped, any other label
    outside [0, C) -> NaN).  totals: None or a device float64 [2] that the forward advances by (loss * counting rows,
    counting rows).  1 <= rows <= 2^22, 2 <= C <= 64 (the library refuses anything else)."""
    _need_gpu(logits, label, weight, totals)
    if logits.dim() < 1 or logits.shape[-1] < 1:
        raise RuntimeError('ops.point_ce: logits [..., C] (got %s)' % (tuple(logits.shape),))
    lead = logits.shape[:-1]
    loss, pred = _PointCE.apply(logits.reshape(-1, logits.shape[-1]), label, weight, ignore_index, totals, bool(want_pred))
    return (loss, pred.view(lead)) if want_pred else loss


def part_iou_state(device):
    """A zeroed state block of sug_part_iou_accumulate (SUG_SEG_STATE_WORDS int64 / fp64 words, held as int64)."""
    return torch.zeros(SEG_STATE_WORDS, dtype=torch.int64, device=device)


def part_iou_state_fields(state):
    """The accumulators of a part-IoU state block (on the host: the one read), as a dict of numpy values."""
    s = state.cpu()
    d = s.view(torch.float64).numpy()
    i = s.numpy()
    K, C = SEG_MAX_CATEGORIES, SEG_MAX_PARTS
    return {'shapes': int(i[SEG_SHAPES]), 'points': int(i[SEG_POINTS]), 'correct': int(i[SEG_CORRECT]), 'error': int(i[SEG_ERROR]),
            'cat_iou': d[SEG_CAT_IOU:SEG_CAT_IOU + K].copy(), 'cat_shapes': i[SEG_CAT_SHAPES:SEG_CAT_SHAPES + K].copy(),
            'part_points': i[SEG_PART_POINTS:SEG_PART_POINTS + C].copy(),
            'part_correct': i[SEG_PART_CORRECT:SEG_PART_CORRECT + C].copy()}


def part_table(part_first, part_count):
    """The categories' part ranges as the two host int32 arrays sug_part_iou_accumulate takes (lists, numpy arrays or CPU
    tensors; they travel by value with every launch, so they are never read back from a device)."""
    import numpy as np
    out = []
    for v in (part_first, part_count):
        if isinstance(v, torch.Tensor):
            if v.is_cuda:
                raise RuntimeError('ops.part_iou_accumulate: part_first / part_count are host arrays (a device tensor would have '
                                   'to be read back)')
            v = v.numpy()
        out.append(np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int32))
    if out[0].shape != out[1].shape:
        raise RuntimeError('ops.part_iou_accumulate: part_first and part_count differ in length')
    return out[0], out[1]


def part_iou_accumulate(logits, label, category, part_first, part_count, state):
    """One batch of the ShapeNet-Part protocol into `state` (sug_part_iou_accumulate): logits [B, N, C] fp32, label [B, N] and
    category [B] int64 on the HIP device; category k owns the parts [part_first[k], part_first[k] + part_count[k]) (host
    arrays, see part_table).  No host synchronisation."""
    _need_gpu(logits, label, category, state)
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise RuntimeError('ops.part_iou_accumulate: fp32 logits [B, N, C] (got %s %s)' % (tuple(logits.shape), logits.dtype))
    B, N, C = logits.shape
    if label.dtype != torch.int64 or label.shape != (B, N) or category.dtype != torch.int64 or category.shape != (B,):
        raise RuntimeError('ops.part_iou_accumulate: label int64 [B, N] and category int64 [B] (got %s %s, %s %s)'
                           % (tuple(label.shape), label.dtype, tuple(category.shape), category.dtype))
    if state.dtype != torch.int64 or state.numel() != SEG_STATE_WORDS or not state.is_contiguous():
        raise RuntimeError('ops.part_iou_accumulate: state is the block ops.part_iou_state() returns')
    first, count = part_table(part_first, part_count)
    records = torch.empty(max(B, 1) * SEG_RECORD_WORDS, dtype=torch.int64, device=logits.device)
    check(lib().sug_part_iou_accumulate(_p(logits.contiguous()), _p(label.contiguous()), _p(category.contiguous()),
                                        first.ctypes.data_as(ctypes.c_void_p), count.ctypes.data_as(ctypes.c_void_p), B, N, C,
                                        first.shape[0], _p(records), _p(state), _st()), 'sug_part_iou_accumulate')


class _SplitHalves(torch.autograd.Function):
    """The two domain halves of a paired [2B, ...] tensor as views.  Backward: when the two gradients are adjacent row
    blocks of one buffer (what mmd_assemble's and the paired kernels' backwards hand back) the pair's gradient is that
    buffer, without the torch.stack / zero fill of unbind's backward."""

    @staticmethod
    def forward(ctx, t):
        B = t.shape[0] // 2
        ctx.meta = (tuple(t.shape), t.dtype, t.device)
        return t[:B], t[B:]

    @staticmethod
    def backward(ctx, ga, gb):
        shape, dtype, dev = ctx.meta
        B = shape[0] // 2
        if ga is not None and gb is not None and ga.shape == gb.shape and ga.stride() == gb.stride() and ga.dim() >= 1 \
                and ga.untyped_storage().data_ptr() == gb.untyped_storage().data_ptr() \
                and gb.storage_offset() == ga.storage_offset() + B * ga.stride(0):
            return torch.as_strided(ga, shape, ga.stride(), ga.storage_offset())
        if ga is None and gb is None:
            return None
        z = lambda: torch.zeros((B,) + shape[1:], dtype=dtype, device=dev)
        return torch.cat((ga if ga is not None else z(), gb if gb is not None else z()), 0)


def split_halves(t):
    """t [2B, ...] -> (t[:B], t[B:]) with a copy-free backward where the producers allow it."""
    return _SplitHalves.apply(t)


# ----------------------------------------------------------------------------- concat without copies
class _AssembleRows(torch.autograd.Function):
    """torch.cat(parts, dim=-1) for parts that (mostly) already live in column slices of `buf`
    [..., sum(widths)]: producers were asked to write there (edgeconv_bn_act_max(out=...)); a part
    stored elsewhere is copied in.  Backward hands every part its column slice of the gradient (views,
    no copies).  `buf` is passed in a list: it is storage, not a differentiable input."""

    @staticmethod
    def forward(ctx, holder, *parts):
        buf = holder[0]
        off, widths = 0, []
        for t in parts:
            w = t.shape[-1]
            dst = buf[..., off:off + w]
            if not (t.data_ptr() == dst.data_ptr() and t.stride() == dst.stride() and t.shape == dst.shape):
                # copy through an alias with its own version counter: an in-place op on a view of `buf`
                # would invalidate (for autograd) the slices the producers already returned
                t2 = t.detach()
                rows = t2.numel() // max(w, 1)
                if t2.is_cuda and t2.dtype == torch.float32 and t2.is_contiguous() and w % 4 == 0 and dst.stride(-1) == 1 \
                        and all(dst.stride(d) == dst.stride(d + 1) * dst.shape[d + 1] for d in range(dst.dim() - 2)) \
                        and dst.stride(-2) % 4 == 0 and t2.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0:
                    # own float4 copy: torch's strided copy kernel takes 30 us for a 16.8 MB part
                    check(lib().sug_copy_rows2d(_p(t2), w, _p(dst), dst.stride(-2), rows, w, _st()), 'sug_copy_rows2d')
                else:
                    alias = torch.empty(0, dtype=buf.dtype, device=buf.device).set_(
                        buf.untyped_storage(), dst.storage_offset(), dst.shape, dst.stride())
                    alias.copy_(t)
            widths.append(w)
            off += w
        if off != buf.shape[-1]:
            raise RuntimeError('assemble_rows: parts cover %d of %d columns' % (off, buf.shape[-1]))
        ctx.widths = widths
        return buf.view(buf.shape)

    @staticmethod
    def backward(ctx, g):
        out, off = [], 0
        for w in ctx.widths:
            out.append(g[..., off:off + w])
            off += w
        return (None,) + tuple(out)


def assemble_rows(buf, parts):
    return _AssembleRows.apply([buf], *parts)


# ----------------------------------------------------------------------------- MMD
_neg_gamma_cache = {}


def _neg_gammas(sigmas, device):
    key = (tuple(float(s) for s in sigmas), str(device))
    if key not in _neg_gamma_cache:
        vals = [-(1.0 / (2 * s ** 2)) for s in sigmas]             # python doubles, model/mmd.py:251
        _neg_gamma_cache[key] = torch.tensor(vals, dtype=torch.float32, device=device)
    return _neg_gamma_cache[key]


class _MixRbfMMD2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, m, w, sigmas, biased=True):
        _need_gpu(Z)
        Zc = Z if (Z.stride(1) == 1 and Z.stride(0) >= Z.shape[1]) else Z.contiguous()
        D = Zc.shape[1]
        dev = Z.device
        ng = _neg_gammas(sigmas, dev)
        need = ctx.needs_input_grad[0]
        wt = torch.empty(2 * m, 2 * m, dtype=torch.float32, device=dev) if need else None
        wc = w.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous() if w is not None else None
        if biased:
            sums = torch.empty(3, dtype=torch.float64, device=dev)
            val = torch.empty((), dtype=torch.float32, device=dev)
            check(lib().sug_mmd_rbf_value(_p(Zc), Zc.stride(0), m, D, _p(wc), _p(ng), len(sigmas), _p(sums), _p(wt), _p(val),
                                          _st()), 'sug_mmd_rbf_value')
        else:
            # _mmd2(biased=False), model/mmd.py:304-308 (no caller in the reference; off the hot path: a few torch ops on
            # the kernel's sums): the diagonals of K_XX / K_YY -- exactly len(sigmas) each, e_ii is identically 0 there and
            # here -- leave the sums, the within-domain pairs are averaged over m (m - 1).  The kernel's gradient weights
            # carry 2 / m^2 for those pairs (their diagonal is already zero): rescaled by m / (m - 1).
            if m < 2:
                raise RuntimeError('mix_rbf_mmd2(biased=False) needs at least two samples per domain')
            sums = torch.zeros(3, dtype=torch.float64, device=dev)
            check(lib().sug_mmd_rbf(_p(Zc), Zc.stride(0), m, D, _p(wc), _p(ng), len(sigmas), _p(sums), _p(wt), _st()), 'sug_mmd_rbf')
            diag = float(len(sigmas) * m)
            val = (((sums[0] - diag) + (sums[1] - diag)) / float(m * (m - 1)) - 2.0 * sums[2] / float(m * m)).to(torch.float32)
            if need:
                r = float(m) / float(m - 1)
                wt[:m, :m] *= r
                wt[m:, m:] *= r
        if need:
            ctx.save_for_backward(Zc, wt)
        return val

    @staticmethod
    def backward(ctx, g):
        Z, wt = ctx.saved_tensors
        M2, D = Z.shape
        gs = g.detach().to(device=Z.device, dtype=torch.float32).reshape(1)
        dZ = torch.empty(M2, D, dtype=torch.float32, device=Z.device)
        check(lib().sug_mmd_rbf_bwd(_p(Z), Z.stride(0), _p(wt), M2 // 2, D, _p(gs), _p(dZ), D, _st()),
              'sug_mmd_rbf_bwd')
        return dZ, None, None, None, None


def mix_rbf_mmd2_rows(Z, m, sample_weights=None, sigmas=SIGMA_LIST, biased=True):
    """Z = cat(X, Y) [2m, D] -> MMD^2 (0-d tensor): the biased estimator (model/mmd.py:300-303) or the unbiased one (:304-308)."""
    return _MixRbfMMD2.apply(Z, m, sample_weights, tuple(sigmas), bool(biased))


class _MixRbfMMD2Sharded(torch.autograd.Function):
    """The global-batch MMD^2 of a batch-sharded step: every rank holds the gathered
    Zall = [X of all ranks ; Y of all ranks] (values only) and evaluates the row block of the kernel
    matrix that belongs to its own samples, rows [row0, row0+mloc) of each domain, against all 2M
    columns (sug_mmd_rbf_rows); the three partial sums cross the ranks as one 3-double all-reduce.
    Backward: the gradient of the own rows comes from the own row block alone
    (sug_mmd_rbf_rows_bwd) -- no collective -- scaled by the world size because the data-parallel
    gradient averaging divides by it again (every rank's loss contains the same global term)."""

    @staticmethod
    def forward(ctx, Zloc, Zall, mloc, M, row0, w, sigmas, world, group):
        import torch.distributed as dist
        _need_gpu(Zloc, Zall)
        Za = Zall if (Zall.stride(1) == 1 and Zall.stride(0) >= Zall.shape[1]) else Zall.contiguous()
        D = Za.shape[1]
        dev = Za.device
        ng = _neg_gammas(sigmas, dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        need = ctx.needs_input_grad[0]
        wt = torch.empty(2 * mloc, 2 * M, dtype=torch.float32, device=dev) if need else None
        wc = w.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous() if w is not None else None
        check(lib().sug_mmd_rbf_rows(_p(Za), Za.stride(0), M, D, _p(wc), _p(ng), len(sigmas), row0, mloc, _p(sums),
                                     _p(wt), _st()), 'sug_mmd_rbf_rows')
        if world > 1:
            dist.all_reduce(sums, group=group)
        if need:
            ctx.save_for_backward(Za, wt)
            ctx.meta = (mloc, M, row0, world)
        mm = float(M) * float(M)
        return ((sums[0] + sums[1] - 2.0 * sums[2]) / mm).float()

    @staticmethod
    def backward(ctx, g):
        Za, wt = ctx.saved_tensors
        mloc, M, row0, world = ctx.meta
        D = Za.shape[1]
        gs = g.detach().to(device=Za.device, dtype=torch.float32).reshape(1)
        dZ = torch.empty(2 * mloc, D, dtype=torch.float32, device=Za.device)
        check(lib().sug_mmd_rbf_rows_bwd(_p(Za), Za.stride(0), _p(wt), M, D, row0, mloc, _p(gs), float(world), _p(dZ), D,
                                         _st()), 'sug_mmd_rbf_rows_bwd')
        return dZ, None, None, None, None, None, None, None, None


def mix_rbf_mmd2_rows_sharded(Zloc, Zall, mloc, M, row0, sample_weights=None, sigmas=SIGMA_LIST, world=1, group=None):
    """Zloc = cat(X_own, Y_own) [2*mloc, D] (differentiable), Zall = cat(X_all, Y_all) [2M, D] (values)."""
    return _MixRbfMMD2Sharded.apply(Zloc, Zall, mloc, M, row0, sample_weights, tuple(sigmas), world, group)


def mmd_rows_local_sums(Zall, M, row0, mloc, sample_weights, sums_out, need_wt=True, sigmas=SIGMA_LIST):
    """First half of mix_rbf_mmd2_rows_sharded for a step whose collectives sit BETWEEN captured graph segments: this
    rank's row block of the kernel matrix of the gathered batch -> its three partial sums accumulated into `sums_out`
    (fp64 [3], zeroed by the caller) and the derivative block wt [2*mloc, 2M]; no collective here."""
    _need_gpu(Zall)
    Za = Zall if (Zall.stride(1) == 1 and Zall.stride(0) >= Zall.shape[1]) else Zall.contiguous()
    D = Za.shape[1]
    ng = _neg_gammas(sigmas, Za.device)
    wt = torch.empty(2 * mloc, 2 * M, dtype=torch.float32, device=Za.device) if need_wt else None
    wc = sample_weights.detach().reshape(-1).to(device=Za.device, dtype=torch.float32).contiguous() \
        if sample_weights is not None else None
    check(lib().sug_mmd_rbf_rows(_p(Za), Za.stride(0), M, D, _p(wc), _p(ng), len(sigmas), row0, mloc, _p(sums_out), _p(wt),
                                 _st()), 'sug_mmd_rbf_rows')
    return Za, wt


class _MMDFromReducedSums(torch.autograd.Function):
    """Second half: the MMD^2 value from the all-reduced sums; the gradient of this rank's rows comes from its own row
    block (sug_mmd_rbf_rows_bwd), scaled by the world size (the gradient averaging divides by it again)."""

    @staticmethod
    def forward(ctx, Zloc, sums, Za, wt, mloc, M, row0, world):
        ctx.save_for_backward(Za, wt)
        ctx.meta = (mloc, M, row0, world)
        mm = float(M) * float(M)
        return ((sums[0] + sums[1] - 2.0 * sums[2]) / mm).float()

    @staticmethod
    def backward(ctx, g):
        Za, wt = ctx.saved_tensors
        mloc, M, row0, world = ctx.meta
        D = Za.shape[1]
        gs = g.detach().to(device=Za.device, dtype=torch.float32).reshape(1)
        dZ = torch.empty(2 * mloc, D, dtype=torch.float32, device=Za.device)
        check(lib().sug_mmd_rbf_rows_bwd(_p(Za), Za.stride(0), _p(wt), M, D, row0, mloc, _p(gs), float(world), _p(dZ), D,
                                         _st()), 'sug_mmd_rbf_rows_bwd')
        return dZ, None, None, None, None, None, None, None


def mmd_from_reduced_sums(Zloc, sums, Za, wt, mloc, M, row0, world):
    return _MMDFromReducedSums.apply(Zloc, sums, Za, wt, mloc, M, row0, world)


class _AssembleZ(torch.autograd.Function):
    """[feat_s ; feat_t | one-hot(label) * scale] of soft_mmd (model/mmd.py:56-66) in one launch instead of
    scatter + three cats + a mul; the gradient of the feature block is handed back as two row-slice views."""

    @staticmethod
    def forward(ctx, feat_s, feat_t, label_s, label_t, scale, num_class):
        _need_gpu(feat_s, feat_t, label_s, label_t)
        m, D = feat_s.shape
        fs = feat_s if feat_s.stride(1) == 1 else feat_s.contiguous()
        ft = feat_t if feat_t.stride(1) == 1 else feat_t.contiguous()
        ls, lt = label_s.reshape(-1).long().contiguous(), label_t.reshape(-1).long().contiguous()
        Z = torch.empty(2 * m, D + num_class, dtype=torch.float32, device=feat_s.device)
        check(lib().sug_mmd_assemble(_p(fs), fs.stride(0), _p(ft), ft.stride(0), _p(ls), _p(lt), m, D, num_class,
                                     float(scale), _p(Z), _st()), 'sug_mmd_assemble')
        ctx.md = (m, D)
        return Z

    @staticmethod
    def backward(ctx, g):
        m, D = ctx.md
        return g[:m, :D], g[m:, :D], None, None, None, None


def mmd_assemble(feat_s, feat_t, label_s, label_t, scale, num_class=10):
    if feat_s.dtype != torch.float32 or feat_t.dtype != torch.float32 or feat_s.shape != feat_t.shape or feat_s.dim() != 2:
        raise RuntimeError('sug_amd.ops.mmd_assemble: two fp32 [m, D] feature blocks of one shape')
    return _AssembleZ.apply(feat_s, feat_t, label_s, label_t, scale, num_class)


class _SoftMMDMulti(torch.autograd.Function):
    """soft_mmd (model/mmd.py:56-66) of up to four (feat_s, feat_t) pairs of ONE batch -- same samples, same labels -- with one
    launch per stage: assemble, kernel sums (+ derivative weights), values; one backward launch (sug_soft_mmd_multi_*).
    Every term's value and gradient equal mmd_assemble + mix_rbf_mmd2_rows of that term bit for bit."""

    @staticmethod
    def forward(ctx, label_s, label_t, scales, ws, sigmas, num_class, *feats):
        n = len(feats) // 2
        _need_gpu(label_s, label_t, *feats)
        m = feats[0].shape[0]
        dev = feats[0].device
        fs = [f if f.stride(1) == 1 else f.contiguous() for f in feats[0::2]]
        ft = [f if f.stride(1) == 1 else f.contiguous() for f in feats[1::2]]
        ls, lt = label_s.reshape(-1).long().contiguous(), label_t.reshape(-1).long().contiguous()
        Ds = [f.shape[1] for f in fs]
        need = [ctx.needs_input_grad[6 + 2 * i] or ctx.needs_input_grad[7 + 2 * i] for i in range(n)]
        Z = [torch.empty(2 * m, D + num_class, dtype=torch.float32, device=dev) for D in Ds]
        wt = [torch.empty(2 * m, 2 * m, dtype=torch.float32, device=dev) if nd else None for nd in need]
        wc = [None if w is None else w.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous() for w in ws]
        for w in wc:
            if w is not None and w.numel() != m:
                raise RuntimeError('soft_mmd_multi: %d sample weights for %d samples' % (w.numel(), m))
        sums = torch.empty(3 * n, dtype=torch.float64, device=dev)
        vals = torch.empty(n, dtype=torch.float32, device=dev)
        ng = _neg_gammas(sigmas, dev)
        I64, I32, F32 = ctypes.c_int64 * n, ctypes.c_int32 * n, ctypes.c_float * n
        check(lib().sug_soft_mmd_multi_fwd(n, _ptrs(fs), I64(*[f.stride(0) for f in fs]), _ptrs(ft), I64(*[f.stride(0) for f in ft]),
                                           I32(*Ds), F32(*[float(v) for v in scales]), _p(ls), _p(lt), m, num_class, _ptrs(wc),
                                           _p(ng), len(sigmas), _ptrs(Z), _ptrs(wt), _p(sums), _p(vals), _st()),
              'sug_soft_mmd_multi_fwd')
        ctx.meta = (n, m, num_class, Ds, need)
        ctx.save_for_backward(*(Z + wt))
        ctx.set_materialize_grads(False)
        return tuple(vals.unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        n, m, num_class, Ds, need = ctx.meta
        saved = ctx.saved_tensors
        Z, wt = saved[:n], saved[n:]
        dev = Z[0].device
        live = [need[i] and gs[i] is not None for i in range(n)]
        gsc = [gs[i].detach().to(device=dev, dtype=torch.float32).reshape(1) if live[i] else None for i in range(n)]
        dZ = [torch.empty(2 * m, Ds[i], dtype=torch.float32, device=dev) if live[i] else None for i in range(n)]
        if any(live):
            check(lib().sug_soft_mmd_multi_bwd(n, _ptrs(Z), (ctypes.c_int32 * n)(*Ds), _ptrs(wt), _ptrs(gsc), m, num_class, _ptrs(dZ),
                                               _st()), 'sug_soft_mmd_multi_bwd')
        out = [None] * 6
        for i in range(n):
            out += [dZ[i][:m] if (live[i] and ctx.needs_input_grad[6 + 2 * i]) else None,
                    dZ[i][m:] if (live[i] and ctx.needs_input_grad[7 + 2 * i]) else None]
        return tuple(out)


def soft_mmd_multi(label_s, label_t, terms, sigmas=SIGMA_LIST, num_class=10):
    """[soft MMD^2 of (feat_s, feat_t, label_weight, sample_weights) for each of `terms`] on one batch (label_s / label_t [m]
    shared by the terms), at most four terms per launch set."""
    terms = list(terms)
    for fs, ft, _, _ in terms:
        if fs.dtype != torch.float32 or ft.dtype != torch.float32 or fs.shape != ft.shape or fs.dim() != 2 \
                or fs.shape[0] != terms[0][0].shape[0]:
            raise RuntimeError('sug_amd.ops.soft_mmd_multi: fp32 [m, D] feature blocks, one m for all terms')
    out = []
    for i in range(0, len(terms), 4):
        grp = terms[i:i + 4]
        feats = [t for fs, ft, _, _ in grp for t in (fs, ft)]
        out += list(_SoftMMDMulti.apply(label_s, label_t, tuple(float(g[2]) for g in grp), tuple(g[3] for g in grp), tuple(sigmas),
                                        int(num_class), *feats))
    return out


CLASS_MMD = _os.environ.get('SUG_CLASS_MMD', '1') != '0'      # A/B knob: 0 = hard_mmd as boolean indexing + mix_rbf_mmd2 (host waits)
CLASS_MMD_MAX_ROWS, CLASS_MMD_MAX_CLASSES, CLASS_MMD_MAX_D = (_H['SUG_CLASS_MMD_MAX_' + _n] for _n in ('ROWS', 'CLASSES', 'D'))
_CLASS_MMD_MODES = {0: 0, 1: 1, 'hard': 0, 'stable': 1}


def _class_select(label_s, label_t, mode, num_class):
    """sug_mmd_select: (idx_s, idx_t, pos_s, pos_t, count), all int32 on the labels' device."""
    _need_gpu(label_s, label_t)
    if mode not in _CLASS_MMD_MODES:
        raise RuntimeError("sug_amd.ops: class pairing mode %r (0 / 'hard', 1 / 'stable')" % (mode,))
    ls, lt = label_s.reshape(-1).long().contiguous(), label_t.reshape(-1).long().contiguous()
    m = ls.numel()
    if lt.numel() != m:
        raise RuntimeError('sug_amd.ops: %d source labels, %d target labels' % (m, lt.numel()))
    buf = torch.empty(4 * m + 1, dtype=torch.int32, device=ls.device)
    idx_s, idx_t, pos_s, pos_t, count = buf[:m], buf[m:2 * m], buf[2 * m:3 * m], buf[3 * m:4 * m], buf[4 * m:]
    check(lib().sug_mmd_select(_p(ls), _p(lt), m, int(num_class), _CLASS_MMD_MODES[mode], _p(idx_s), _p(idx_t), _p(pos_s),
                               _p(pos_t), _p(count), _st()), 'sug_mmd_select')
    return idx_s, idx_t, pos_s, pos_t, count


def class_pairs(label_s, label_t, mode, num_class=10):
    """The rows that the class-aligned MMD pairs, chosen on the device: (idx_s, idx_t, n) -- int32 [m] row lists whose first
    n entries are valid (-1 after them) and the 0-d int32 count n; nothing is read back.  mode 0 / 'hard' (hard_mmd,
    model/mmd.py:69-77): the rows with label_s[i] == label_t[i] in ascending order, idx_s == idx_t.  mode 1 / 'stable': for
    every class c in ascending order the first min(a_c, b_c) rows of class c of each domain, lowest index first -- the
    counts of get_most_overlapped_element (utils/common_utils.py), with a defined choice of members.  A label outside
    [0, num_class) is never paired, on either side, and raises nothing (the reference asserts on a large source label and
    silently ignores the others).  1 <= m <= 1024, 1 <= num_class <= 64.  mmd.class_pairs_host restates the rules."""
    idx_s, idx_t, _, _, count = _class_select(label_s, label_t, mode, num_class)
    return idx_s, idx_t, count.reshape(())


class _ClassMMD(torch.autograd.Function):
    """mix_rbf_mmd2(feat_s[idx_s[:n]], feat_t[idx_t[:n]]) for the rows of class_pairs, with n left on the device: every
    buffer is sized by m, the kernels read n (sug_class_mmd_*).  Per-pair arithmetic and backward body are those of
    mix_rbf_mmd2_rows on the gathered rows; unselected rows get exact zeros; n == 0 gives NaN with zero gradients."""

    @staticmethod
    def forward(ctx, feat_s, feat_t, label_s, label_t, mode, sigmas, num_class):
        _need_gpu(feat_s, feat_t, label_s, label_t)
        m, D = feat_s.shape
        dev = feat_s.device
        fs = feat_s if (feat_s.stride(1) == 1 and feat_s.stride(0) >= D) else feat_s.contiguous()
        ft = feat_t if (feat_t.stride(1) == 1 and feat_t.stride(0) >= D) else feat_t.contiguous()
        idx_s, idx_t, pos_s, pos_t, count = _class_select(label_s, label_t, mode, num_class)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        Z = torch.empty(2 * m, D, dtype=torch.float32, device=dev)
        wt = torch.empty(2 * m, 2 * m, dtype=torch.float32, device=dev) if need else None
        sums = torch.empty(3, dtype=torch.float64, device=dev)
        val = torch.empty((), dtype=torch.float32, device=dev)
        ng = _neg_gammas(sigmas, dev)
        check(lib().sug_class_mmd_fwd(_p(fs), fs.stride(0), _p(ft), ft.stride(0), m, D, _p(idx_s), _p(idx_t), _p(count), _p(ng),
                                      len(sigmas), _p(Z), _p(wt), _p(sums), _p(val), _st()), 'sug_class_mmd_fwd')
        if need:
            ctx.save_for_backward(Z, wt, count, pos_s, pos_t)
        return val

    @staticmethod
    def backward(ctx, g):
        Z, wt, count, pos_s, pos_t = ctx.saved_tensors
        m, D = Z.shape[0] // 2, Z.shape[1]
        gs = g.detach().to(device=Z.device, dtype=torch.float32).reshape(1)
        dZ = torch.empty(2 * m, D, dtype=torch.float32, device=Z.device)
        dF = torch.empty(2 * m, D, dtype=torch.float32, device=Z.device)      # [d feat_s ; d feat_t], written entirely
        check(lib().sug_class_mmd_bwd(_p(Z), _p(wt), m, D, _p(count), _p(pos_s), _p(pos_t), _p(gs), _p(dZ), _p(dF), D, _p(dF[m:]),
                                      D, _st()), 'sug_class_mmd_bwd')
        return (dF[:m] if ctx.needs_input_grad[0] else None, dF[m:] if ctx.needs_input_grad[1] else None,
                None, None, None, None, None)


def class_mmd_supported(label_s, feat_s, label_t, feat_t, sigmas=SIGMA_LIST, num_class=10):
    """What class_mmd takes (and sug_class_mmd_* would otherwise refuse), and the SUG_CLASS_MMD knob: two fp32 [m, D] feature
    blocks of one shape and m integer labels per domain on the HIP device, 1 <= m <= 1024, 1 <= D <= 2^20,
    1 <= num_class <= 64, 1 to 8 sigmas."""
    if not CLASS_MMD:
        return False
    ts = (label_s, feat_s, label_t, feat_t)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        return False
    if feat_s.dtype != torch.float32 or feat_t.dtype != torch.float32 or feat_s.dim() != 2 or feat_s.shape != feat_t.shape:
        return False
    m, D = feat_s.shape
    for lab in (label_s, label_t):
        if lab.numel() != m or lab.is_floating_point() or lab.is_complex() or lab.dtype == torch.bool:
            return False
    return 1 <= m <= CLASS_MMD_MAX_ROWS and 1 <= D <= CLASS_MMD_MAX_D and 1 <= int(num_class) <= CLASS_MMD_MAX_CLASSES \
        and 1 <= len(sigmas) <= 8


def class_mmd(label_s, feat_s, label_t, feat_t, mode, sigmas=SIGMA_LIST, num_class=10):
    """Class-aligned MMD^2 (0-d fp32 tensor, differentiable in both feature blocks) of the rows class_pairs selects: mode 0 /
    'hard' is hard_mmd (model/mmd.py:69-77), mode 1 / 'stable' max_hard_mmd (:96-104) with the stable pairing.  No host
    read, no boolean indexing: a step that calls it can be captured, and one captured step serves batches with different
    n.  No pair (n == 0): NaN, and both gradients exact zeros, as the reference has it."""
    if feat_s.dtype != torch.float32 or feat_t.dtype != torch.float32 or feat_s.shape != feat_t.shape or feat_s.dim() != 2:
        raise RuntimeError('sug_amd.ops.class_mmd: two fp32 [m, D] feature blocks of one shape')
    if not 1 <= len(sigmas) <= 8:
        raise RuntimeError('sug_amd.ops.class_mmd: 1 to 8 sigmas (got %d)' % len(sigmas))
    return _ClassMMD.apply(feat_s, feat_t, label_s, label_t, mode, tuple(sigmas), int(num_class))


MMD_EST_MAX_ROWS, MMD_EST_MAX_D, MMD_EST_MAX_SIGMAS, MMD_POLY_MAX_DEGREE = (
    _H['SUG_MMD_' + _n] for _n in ('EST_MAX_ROWS', 'EST_MAX_D', 'EST_MAX_SIGMAS', 'POLY_MAX_DEGREE'))


def _unit_rows(t):
    """A 2-d fp32 tensor as rows with unit column stride (a column slice stays a view; anything else is copied)."""
    return t if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) else t.contiguous()


class _MMDRatio(torch.autograd.Function):
    """(loss, mmd2, var_est) of Z = [X ; Y] in four launches (sug_mmd_ratio_fwd), the gradient of any combination of the
    three in one (sug_mmd_ratio_bwd): the factors of the two saved weight matrices are formed on the device from the three
    upstream gradients and the forward's own outputs."""

    @staticmethod
    def forward(ctx, Z, m, sigmas, biased):
        _need_gpu(Z)
        Zc = _unit_rows(Z)
        D, dev = Zc.shape[1], Z.device
        M2 = 2 * m
        ng = _neg_gammas(sigmas, dev)
        need = ctx.needs_input_grad[0]
        f32 = dict(dtype=torch.float32, device=dev)
        KG = torch.empty(2, M2, M2, **f32)
        wt = torch.empty(2, M2, M2, **f32) if need else None
        rows = torch.empty(_H['SUG_MMD_RATIO_ROW_FIELDS'] * m, dtype=torch.float64, device=dev)
        stats = torch.empty(_H['SUG_MMD_RATIO_STATS'], dtype=torch.float64, device=dev)
        out3 = torch.empty(3, **f32)
        check(lib().sug_mmd_ratio_fwd(_p(Zc), Zc.stride(0), m, D, _p(ng), len(sigmas), int(bool(biased)), _p(KG[0]), _p(KG[1]),
                                      _p(rows), _p(stats), _p(out3), _p(wt[0]) if need else None, _p(wt[1]) if need else None,
                                      _st()), 'sug_mmd_ratio_fwd')
        if need:
            ctx.save_for_backward(Zc, wt, out3)
        return out3[0], out3[1], out3[2]

    @staticmethod
    def backward(ctx, g_loss, g_mmd2, g_var):
        Z, wt, out3 = ctx.saved_tensors
        M2, D = Z.shape
        g3 = torch.stack((g_loss.detach().reshape(()), g_mmd2.detach().reshape(()), g_var.detach().reshape(()))).to(
            device=Z.device, dtype=torch.float32)
        dZ = torch.empty(M2, D, dtype=torch.float32, device=Z.device)
        check(lib().sug_mmd_ratio_bwd(_p(Z), Z.stride(0), M2 // 2, D, _p(wt[0]), _p(wt[1]), _p(out3), _p(g3), _p(dZ), D, _st()),
              'sug_mmd_ratio_bwd')
        return dZ, None, None, None


def _fp32_rows_pair(X, Y):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 for t in (X, Y)) \
        and X.shape == Y.shape and 2 <= X.shape[0] <= MMD_EST_MAX_ROWS and 1 <= X.shape[1] <= MMD_EST_MAX_D


def mmd_ratio_supported(X, Y, sigmas=SIGMA_LIST):
    """What mmd_ratio takes of the two domains' blocks (and sug_mmd_ratio_* would otherwise refuse): fp32 [m, D] of one
    shape on the HIP device, 2 <= m <= 1024, 1 <= D <= 2^20, 1 to 8 sigmas."""
    return _fp32_rows_pair(X, Y) and 1 <= len(sigmas) <= MMD_EST_MAX_SIGMAS


def mmd_ratio(Z, m, sigmas=SIGMA_LIST, biased=True):
    """Z = cat(X, Y) [2m, D] -> (loss, mmd2, var_est), 0-d fp32 tensors, differentiable in Z: the MMD^2 of the Gaussian
    multi-kernel matrix (biased or unbiased), the estimate of its variance, and mmd2 / sqrt(max(var_est, 1e-8))
    (_mmd2_and_ratio, model/mmd.py:315-373).  The row and scalar sums are folded in fp64 in a fixed order."""
    if Z.dtype != torch.float32 or Z.dim() != 2 or Z.shape[0] != 2 * m:
        raise RuntimeError('sug_amd.ops.mmd_ratio: Z = cat(X, Y), fp32 [2m, D]')
    if not 2 <= m <= MMD_EST_MAX_ROWS:
        raise RuntimeError('sug_amd.ops.mmd_ratio: m=%d rows per domain (2..%d)' % (m, MMD_EST_MAX_ROWS))
    if not 1 <= len(sigmas) <= MMD_EST_MAX_SIGMAS:
        raise RuntimeError('sug_amd.ops.mmd_ratio: 1 to %d sigmas (got %d)' % (MMD_EST_MAX_SIGMAS, len(sigmas)))
    return _MMDRatio.apply(Z, int(m), tuple(sigmas), bool(biased))


class _AdjacentMMD(torch.autograd.Function):
    """linear_mmd2 (mode 0) / poly_mmd2 (mode 1) over the m - 1 adjacent row pairs (sug_mmd_adjacent_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, X, Y, mode, degree, alpha, c):
        _need_gpu(X, Y)
        Xc, Yc = _unit_rows(X), _unit_rows(Y)
        m, D = Xc.shape
        dev = X.device
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        part = torch.empty(m - 1, dtype=torch.float64, device=dev)
        coef = torch.empty(4, m - 1, dtype=torch.float32, device=dev) if (need and mode == 1) else None
        val = torch.empty((), dtype=torch.float32, device=dev)
        check(lib().sug_mmd_adjacent_fwd(_p(Xc), Xc.stride(0), _p(Yc), Yc.stride(0), m, D, mode, degree, alpha, c, _p(part),
                                         _p(coef), _p(val), _st()), 'sug_mmd_adjacent_fwd')
        if need:
            ctx.mode = mode
            ctx.save_for_backward(Xc, Yc, coef)
        return val

    @staticmethod
    def backward(ctx, g):
        X, Y, coef = ctx.saved_tensors
        m, D = X.shape
        gs = g.detach().to(device=X.device, dtype=torch.float32).reshape(1)
        d = torch.empty(2, m, D, dtype=torch.float32, device=X.device)
        check(lib().sug_mmd_adjacent_bwd(_p(X), X.stride(0), _p(Y), Y.stride(0), m, D, ctx.mode, _p(coef), _p(gs), _p(d[0]), D,
                                         _p(d[1]), D, _st()), 'sug_mmd_adjacent_bwd')
        return (d[0] if ctx.needs_input_grad[0] else None, d[1] if ctx.needs_input_grad[1] else None, None, None, None, None)


def adjacent_mmd_supported(X, Y, d=1):
    """What linear_mmd2 / poly_mmd2 take: two fp32 [m, D] blocks of one shape on the HIP device, 2 <= m <= 1024,
    1 <= D <= 2^20, and an integer degree in 1..8."""
    return _fp32_rows_pair(X, Y) and not isinstance(d, bool) and isinstance(d, (int, float)) and float(d).is_integer() \
        and 1 <= int(d) <= MMD_POLY_MAX_DEGREE


def _adjacent(name, X, Y, mode, d, alpha, c):
    if not adjacent_mmd_supported(X, Y, d):
        _need_gpu(*(t for t in (X, Y) if isinstance(t, torch.Tensor)))
        raise RuntimeError('sug_amd.ops.%s: two fp32 [m, D] blocks of one shape, 2 <= m <= %d, 1 <= D <= %d, an integer degree '
                           'in 1..%d' % (name, MMD_EST_MAX_ROWS, MMD_EST_MAX_D, MMD_POLY_MAX_DEGREE))
    return _AdjacentMMD.apply(X, Y, mode, int(d), float(alpha), float(c))


def linear_mmd2(X, Y):
    """mean_i <x_i - y_i, x_{i+1} - y_{i+1}> (model/mmd.py:211-216): the linear-time MMD^2 with the linear kernel, 0-d fp32,
    differentiable in both blocks."""
    return _adjacent('linear_mmd2', X, Y, 0, 1, 1.0, 0.0)


def poly_mmd2(X, Y, d=2, alpha=1.0, c=2.0):
    """The linear-time MMD^2 with the kernel (alpha <x, y> + c)^d over adjacent rows (model/mmd.py:223-236)."""
    return _adjacent('poly_mmd2', X, Y, 1, d, alpha, c)


CL_LOSS = _os.environ.get('SUG_CL_LOSS', '1') != '0'          # A/B knob: 0 = the composed lines of mmd.contrastive_loss_weighted
CL_LOSS_MAX_ROWS, CL_LOSS_MAX_D, CL_LOSS_MAX_TERMS = (_H['SUG_CL_LOSS_MAX_' + _n] for _n in ('ROWS', 'D', 'TERMS'))


def _cl_weights(w, m, dev):
    if w is None:
        return None
    wc = w.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    if wc.numel() != m:
        raise RuntimeError('sug_amd.ops.cl_loss: %d sample weights for %d samples' % (wc.numel(), m))
    return wc


def _cl_forward(label_s, label_t, margins, ws, fs, ft, need):
    """sug_cl_loss_fwd of the terms (fs[i], ft[i]): (values fp32 [n], coef: fp64 [4, m] per term with need[i], else None)."""
    n, m, dev = len(fs), fs[0].shape[0], fs[0].device
    ls, lt = label_s.reshape(-1).contiguous(), label_t.reshape(-1).contiguous()
    wc = [_cl_weights(w, m, dev) for w in ws]
    sums = torch.empty(n * _H['SUG_CL_LOSS_SUM_FIELDS'] * m, dtype=torch.float64, device=dev)
    coef = [torch.empty(_H['SUG_CL_LOSS_ROW_FIELDS'], m, dtype=torch.float64, device=dev) if nd else None for nd in need]
    vals = torch.empty(n, dtype=torch.float32, device=dev)
    I64, I32, F64 = ctypes.c_int64 * n, ctypes.c_int32 * n, ctypes.c_double * n
    check(lib().sug_cl_loss_fwd(n, _ptrs(fs), I64(*[f.stride(0) for f in fs]), _ptrs(ft), I64(*[f.stride(0) for f in ft]),
                                I32(*[f.shape[1] for f in fs]), F64(*[float(v) for v in margins]), _p(ls), _p(lt), m, _ptrs(wc),
                                _p(sums), _ptrs(coef), _p(vals), _st()), 'sug_cl_loss_fwd')
    return vals, coef


class _CLLossMulti(torch.autograd.Function):
    """The weighted cosine-embedding loss (contrastive_loss_weighted, model/mmd.py:80-94) of up to four (feat_s, feat_t)
    pairs of ONE batch -- same rows, same labels: two launches forward for all of them, one backward (sug_cl_loss_*).  A
    term's value and gradient do not depend on the terms beside it."""

    @staticmethod
    def forward(ctx, label_s, label_t, margins, ws, *feats):
        n = len(feats) // 2
        _need_gpu(label_s, label_t, *feats)
        fs, ft = [_unit_rows(f) for f in feats[0::2]], [_unit_rows(f) for f in feats[1::2]]
        need = [ctx.needs_input_grad[4 + 2 * i] or ctx.needs_input_grad[5 + 2 * i] for i in range(n)]
        vals, coef = _cl_forward(label_s, label_t, margins, ws, fs, ft, need)
        ctx.need = need
        ctx.save_for_backward(*(fs + ft + coef))
        ctx.set_materialize_grads(False)
        return tuple(vals.unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        need, n = ctx.need, len(ctx.need)
        saved = ctx.saved_tensors
        fs, ft, coef = saved[:n], saved[n:2 * n], saved[2 * n:]
        dev = fs[0].device
        m = fs[0].shape[0]
        live = [need[i] and gs[i] is not None for i in range(n)]
        gsc = [gs[i].detach().to(device=dev, dtype=torch.float32).reshape(1) if live[i] else None for i in range(n)]
        dx = [torch.empty_like(fs[i], memory_format=torch.contiguous_format) if (live[i] and ctx.needs_input_grad[4 + 2 * i]) else None
              for i in range(n)]
        dy = [torch.empty_like(ft[i], memory_format=torch.contiguous_format) if (live[i] and ctx.needs_input_grad[5 + 2 * i]) else None
              for i in range(n)]
        if any(live):
            Ds = [f.shape[1] for f in fs]
            I64, I32 = ctypes.c_int64 * n, ctypes.c_int32 * n
            check(lib().sug_cl_loss_bwd(n, _ptrs(fs), I64(*[f.stride(0) for f in fs]), _ptrs(ft), I64(*[f.stride(0) for f in ft]),
                                        I32(*Ds), m, _ptrs(coef), _ptrs(gsc), _ptrs(dx), I64(*Ds), _ptrs(dy), I64(*Ds), _st()),
                  'sug_cl_loss_bwd')
        out = [None] * 4
        for i in range(n):
            out += [dx[i], dy[i]]
        return tuple(out)


def cl_loss_supported(label_s, feat_s, label_t, feat_t, margin=0.2, sample_weights=None):
    """What cl_loss takes (and sug_cl_loss_* would otherwise refuse), and the SUG_CL_LOSS knob: two fp32 [m, D] feature blocks
    of one shape and m int64 labels per domain (1-D) on the HIP device, 1 <= m <= 1024, 1 <= D <= 2^20, a finite margin, and
    sample weights -- constants here -- that do not require grad and have m elements after squeeze."""
    if not CL_LOSS:
        return False
    ts = (label_s, feat_s, label_t, feat_t)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        return False
    if feat_s.dtype != torch.float32 or feat_t.dtype != torch.float32 or feat_s.dim() != 2 or feat_s.shape != feat_t.shape:
        return False
    m, D = feat_s.shape
    for lab in (label_s, label_t):
        if lab.dtype != torch.int64 or lab.dim() != 1 or lab.numel() != m:
            return False
    if sample_weights is not None:
        if not isinstance(sample_weights, torch.Tensor) or sample_weights.requires_grad or not sample_weights.is_floating_point():
            return False
        sq = sample_weights.squeeze()
        if sq.numel() != m or sq.dim() > 1:
            return False
    try:
        finite = math.isfinite(float(margin))
    except (TypeError, ValueError):
        return False
    return finite and 1 <= m <= CL_LOSS_MAX_ROWS and 1 <= D <= CL_LOSS_MAX_D


def cl_loss_multi(label_s, label_t, terms):
    """[cl_loss of (feat_s, feat_t, margin, sample_weights) for each of `terms`] on one batch (label_s / label_t int64 [m]
    shared by the terms), at most four terms per launch set; each value and gradient has the bits of its own cl_loss call."""
    terms = list(terms)
    for fs, ft, margin, w in terms:
        if not cl_loss_supported(label_s, fs, label_t, ft, margin, w):
            _need_gpu(*(t for t in (label_s, fs, label_t, ft) if isinstance(t, torch.Tensor)))
            raise RuntimeError('sug_amd.ops.cl_loss: two fp32 [m, D] feature blocks of one shape, int64 labels [m], 1 <= m <= %d, '
                               '1 <= D <= %d, a finite margin, constant sample weights with m elements%s'
                               % (CL_LOSS_MAX_ROWS, CL_LOSS_MAX_D, '' if CL_LOSS else ' (and not with SUG_CL_LOSS=0)'))
    out = []
    for i in range(0, len(terms), CL_LOSS_MAX_TERMS):
        grp = terms[i:i + CL_LOSS_MAX_TERMS]
        feats = [t for fs, ft, _, _ in grp for t in (fs, ft)]
        out += list(_CLLossMulti.apply(label_s, label_t, tuple(float(g[2]) for g in grp), tuple(g[3] for g in grp), *feats))
    return out


def cl_loss(label_s, feat_s, label_t, feat_t, margin=0.2, sample_weights=None):
    """mean_i w_i l_i with l_i = 1 - cos(x_i, y_i) where label_s[i] == label_t[i] and max(0, cos - margin) elsewhere
    (contrastive_loss_weighted with nn.CosineEmbeddingLoss(margin, reduction='none'), model/mmd.py:80-94): 0-d fp32,
    differentiable in both feature blocks; the weights are constants.  Sums in fp64 in a fixed order."""
    return cl_loss_multi(label_s, label_t, [(feat_s, feat_t, margin, sample_weights)])[0]


def cl_loss_cos(feat_s, feat_t):
    """The rows' cosines as cl_loss forms them, fp64 [m] (the fold's saved field): what a row contributes depends on that
    row alone."""
    lab = torch.zeros(feat_s.shape[0], dtype=torch.int64, device=feat_s.device)
    if not cl_loss_supported(lab, feat_s, lab, feat_t):
        raise RuntimeError('sug_amd.ops.cl_loss_cos: two fp32 [m, D] feature blocks of one shape on the HIP device')
    _, coef = _cl_forward(lab, lab, (0.0,), (None,), [_unit_rows(feat_s.detach())], [_unit_rows(feat_t.detach())], [True])
    return coef[0][_H['SUG_CL_LOSS_ROW_FIELDS'] - 1]


def colsum(x2, sign=1.0):
    """fp32 column sums [C] of a [R, C] fp32 / fp16 matrix (sug_colsum: no memset, fixed order)."""
    _need_gpu(x2)
    if x2.dim() != 2 or x2.dtype not in (torch.float32, torch.float16):
        raise RuntimeError('sug_amd.ops.colsum: a 2-D fp32 / fp16 matrix')
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    R, C = x2.shape
    out = torch.empty(C, dtype=torch.float32, device=x2.device)
    ws = torch.empty(int(lib().sug_colsum_workspace(R, C)), dtype=torch.float32, device=x2.device)
    check(lib().sug_colsum(_p(x2), x2.stride(0), R, C, 0 if x2.dtype == torch.float32 else 1, float(sign), _p(out), _p(ws),
                           _st()), 'sug_colsum')
    return out


class _SubRowBias(torch.autograd.Function):
    """rows [..., C] - bias [C]; the bias gradient by sug_colsum instead of autograd's sum_to_size."""

    @staticmethod
    def forward(ctx, rows, bias):
        return rows - bias

    @staticmethod
    def backward(ctx, g):
        db = colsum(g.reshape(-1, g.shape[-1]), -1.0) if ctx.needs_input_grad[1] else None
        return g, db


def sub_row_bias(rows, bias):
    return _SubRowBias.apply(rows, bias)


class _Gate(torch.autograd.Function):
    """x * sigmoid(z) + x (CALayer, model/Model.py:28-34) in one launch forward and one backward instead of
    sigmoid / mul / add and their four backward launches."""

    @staticmethod
    def forward(ctx, x, z):
        _need_gpu(x, z)
        x, z = x.contiguous(), z.contiguous()
        out = torch.empty_like(x)
        check(lib().sug_gate_fwd(_p(x), _p(z), x.numel(), _p(out), _st()), 'sug_gate_fwd')
        ctx.save_for_backward(x, z)
        return out

    @staticmethod
    def backward(ctx, g):
        x, z = ctx.saved_tensors
        g = g.contiguous()
        dx, dz = torch.empty_like(x), torch.empty_like(x)
        check(lib().sug_gate_bwd(_p(g), _p(x), _p(z), x.numel(), _p(dx), _p(dz), _st()), 'sug_gate_bwd')
        return dx, dz


def gate(x, z):
    if x.dtype != torch.float32 or z.dtype != torch.float32 or x.shape != z.shape:
        raise RuntimeError('sug_amd.ops.gate: two fp32 tensors of one shape')
    return _Gate.apply(x, z)


class _GateBN(torch.autograd.Function):
    """BatchNorm1d(x * sigmoid(z) + x) over the M rows of x, z [M, C] -- the tail of CALayer (sug_gate_bn_fwd / _bwd):
    one launch each way instead of the gate + torch's three BatchNorm launches (and its 32 us backward reduce)."""

    @staticmethod
    def forward(ctx, x, z, gamma, beta, running_mean, running_var, training, eps, momentum):
        _need_gpu(x, z, gamma)
        x, z = x.contiguous(), z.contiguous()
        M, C = x.shape
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        out = torch.empty_like(x)
        stat = torch.empty(2, C, dtype=torch.float32, device=x.device)
        check(lib().sug_gate_bn_fwd(_p(x), _p(z), M, C, _p(g), _p(b), _p(running_mean), _p(running_var), 1 if training else 0,
                                    float(eps), float(momentum), _p(out), _p(stat), _st()), 'sug_gate_bn_fwd')
        ctx.save_for_backward(x, z, g, stat)
        ctx.training = bool(training)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, z, g, stat = ctx.saved_tensors
        M, C = x.shape
        gout = gout.contiguous()
        dx, dz = torch.empty_like(x), torch.empty_like(x)
        dgb = torch.empty(2, C, dtype=torch.float32, device=x.device)
        check(lib().sug_gate_bn_bwd(_p(gout), _p(x), _p(z), M, C, _p(g), _p(stat), 1 if ctx.training else 0, _p(dx), _p(dz),
                                    _p(dgb[0]), _p(dgb[1]), _st()), 'sug_gate_bn_bwd')
        return dx, dz, dgb[0], dgb[1], None, None, None, None, None


GATE_BN_FUSED = _os.environ.get('SUG_GATE_BN_FUSED', '1') != '0'


def gate_bn_supported(x, bn):
    return GATE_BN_FUSED and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] <= 1024 and bn.affine and \
        (bn.training or bn.track_running_stats) and bn.momentum is not None and CTX.bn_groups == 1


def gate_bn(x, z, bn):
    """bn(x * sigmoid(z) + x) for an nn.BatchNorm1d over [M, C] rows (CALayer, model/Model.py:28-34)."""
    if x.dtype != torch.float32 or z.dtype != torch.float32 or x.shape != z.shape:
        raise RuntimeError('sug_amd.ops.gate_bn: two fp32 tensors of one shape')
    _count_bn_call(bn)
    track = bn.track_running_stats
    return _GateBN.apply(x, z, bn.weight, bn.bias, bn.running_mean if track else None, bn.running_var if track else None,
                         bn.training or not track, bn.eps, bn.momentum)


class _EdgeWeightSplit(torch.autograd.Function):
    """W [Co, 2C] -> [W1 ; W2 - W1] [2Co, C], the EdgeConv GEMM operand (one launch forward, one backward:
    dW = [gP - gQ | gQ])."""

    @staticmethod
    def forward(ctx, W):
        _need_gpu(W)
        W = W.contiguous()
        Co, C = W.shape[0], W.shape[1] // 2
        out = torch.empty(2 * Co, C, dtype=torch.float32, device=W.device)
        check(lib().sug_edge_weight_split(_p(W), Co, C, 0, _p(out), _st()), 'sug_edge_weight_split')
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        Co, C = g.shape[0] // 2, g.shape[1]
        dW = torch.empty(Co, 2 * C, dtype=torch.float32, device=g.device)
        check(lib().sug_edge_weight_split(_p(g), Co, C, 1, _p(dW), _st()), 'sug_edge_weight_split')
        return dW


def edge_weight_split(W):
    if W.dtype != torch.float32 or W.dim() != 2 or W.shape[1] % 2:
        raise RuntimeError('sug_amd.ops.edge_weight_split: fp32 [Co, 2C] weight')
    return _EdgeWeightSplit.apply(W)


class _EdgeWeightSplitMulti(torch.autograd.Function):
    """_EdgeWeightSplit for several weights at once: one launch forward, one backward (sug_edge_weight_split_multi); a
    split that received no gradient hands None to its weight."""

    @staticmethod
    def forward(ctx, *Ws):
        _need_gpu(*Ws)
        Ws = [W.contiguous() for W in Ws]
        n = len(Ws)
        ctx.shapes = [(W.shape[0], W.shape[1] // 2) for W in Ws]
        outs = [torch.empty(2 * Co, C, dtype=torch.float32, device=W.device) for W, (Co, C) in zip(Ws, ctx.shapes)]
        I32 = ctypes.c_int32 * n
        check(lib().sug_edge_weight_split_multi(_ptrs(Ws), I32(*[s[0] for s in ctx.shapes]), I32(*[s[1] for s in ctx.shapes]), n, 0,
                                                _ptrs(outs), _st()), 'sug_edge_weight_split_multi')
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        n = len(gs)
        gs = [None if (g is None or not ctx.needs_input_grad[i]) else g.contiguous() for i, g in enumerate(gs)]
        if all(g is None for g in gs):
            return (None,) * n
        dev = next(g for g in gs if g is not None).device
        dWs = [None if g is None else torch.empty(Co, 2 * C, dtype=torch.float32, device=dev) for g, (Co, C) in zip(gs, ctx.shapes)]
        I32 = ctypes.c_int32 * n
        check(lib().sug_edge_weight_split_multi(_ptrs(gs), I32(*[s[0] for s in ctx.shapes]), I32(*[s[1] for s in ctx.shapes]), n, 1,
                                                _ptrs(dWs), _st()), 'sug_edge_weight_split_multi')
        return tuple(dWs)


def edge_weight_split_multi(Ws):
    """[edge_weight_split(W) for W in Ws] in one launch each way (at most 8 weights per launch)."""
    Ws = list(Ws)
    for W in Ws:
        if W.dtype != torch.float32 or W.dim() != 2 or W.shape[1] % 2:
            raise RuntimeError('sug_amd.ops.edge_weight_split_multi: fp32 [Co, 2C] weights')
    if len(Ws) == 1:
        return [_EdgeWeightSplit.apply(Ws[0])]
    out = []
    for i in range(0, len(Ws), 8):
        out += list(_EdgeWeightSplitMulti.apply(*Ws[i:i + 8]))
    return out


_SDA_METHODS = {'none': 0, 'naive_inverse': 1, 'exp_inverse': 2, 'mean2one': 3}


SDA_MAX_CLASSES = _H['SUG_SDA_MAX_CLASSES']


def _sda_num_class(*preds):
    """The class count of SDA logits: their common width (the kernel states its own range, 2..SDA_MAX_CLASSES)."""
    C = int(preds[0].shape[-1])
    if any(int(p.shape[-1]) != C for p in preds):
        raise RuntimeError('sda_prob_weights: logits of one width (got %s)' % sorted({int(p.shape[-1]) for p in preds}))
    return C


def sda_prob_weights(pred_s, pred_t, label_s, label_t, label_weight, method):
    """SDA weights [m] from logits [m,C] and labels [m] (prob_weights_soft + distance2weights,
    model/mmd.py:134-148, :178-202) in one kernel.  C = the logits' width, 2..SDA_MAX_CLASSES (the reference: 10).  A label
    outside [0, C) gets no one-hot entry and raises nothing."""
    _need_gpu(pred_s, pred_t, label_s, label_t)
    if method not in _SDA_METHODS:
        raise RuntimeError('Not supported weighting method %s' % method)
    C = _sda_num_class(pred_s, pred_t)
    ps = pred_s.detach().reshape(-1, C).float()
    pt = pred_t.detach().reshape(-1, C).float()
    ps = ps if ps.stride(1) == 1 else ps.contiguous()
    pt = pt if pt.stride(1) == 1 else pt.contiguous()
    ls, lt = label_s.reshape(-1).long().contiguous(), label_t.reshape(-1).long().contiguous()
    m = ps.shape[0]
    out = torch.empty(m, dtype=torch.float32, device=ps.device)
    check(lib().sug_sda_prob_weights(_p(ps), ps.stride(0), _p(pt), pt.stride(0), _p(ls), _p(lt), m, C,
                                     float(label_weight), _SDA_METHODS[method], _p(out), _st()),
          'sug_sda_prob_weights')
    return out


def sda_prob_weights_multi(preds, label_s, label_t, label_weight, method):
    """[sda_prob_weights(ps, pt, ...) for (ps, pt) in preds] in one launch (at most four heads; one batch, one set of labels)."""
    preds = list(preds)
    if len(preds) == 1:
        return [sda_prob_weights(preds[0][0], preds[0][1], label_s, label_t, label_weight, method)]
    if len(preds) > 4:
        return sda_prob_weights_multi(preds[:4], label_s, label_t, label_weight, method) + \
            sda_prob_weights_multi(preds[4:], label_s, label_t, label_weight, method)
    if method not in _SDA_METHODS:
        raise RuntimeError('Not supported weighting method %s' % method)
    C = _sda_num_class(*[t for pr in preds for t in pr])
    rows = lambda p: (lambda q: q if q.stride(1) == 1 else q.contiguous())(p.detach().reshape(-1, C).float())
    ps, pt = [rows(a) for a, _ in preds], [rows(b) for _, b in preds]
    _need_gpu(label_s, label_t, *(ps + pt))
    ls, lt = label_s.reshape(-1).long().contiguous(), label_t.reshape(-1).long().contiguous()
    m, n = ps[0].shape[0], len(preds)
    if any(t.shape[0] != m for t in ps + pt):
        raise RuntimeError('sda_prob_weights_multi: one batch size for all heads')
    outs = [torch.empty(m, dtype=torch.float32, device=ps[0].device) for _ in range(n)]
    I64 = ctypes.c_int64 * n
    check(lib().sug_sda_prob_weights_multi(n, _ptrs(ps), I64(*[t.stride(0) for t in ps]), _ptrs(pt), I64(*[t.stride(0) for t in pt]),
                                           _p(ls), _p(lt), m, C, float(label_weight), _SDA_METHODS[method], _ptrs(outs), _st()),
          'sug_sda_prob_weights_multi')
    return outs


CHAMFER_MERGED = _os.environ.get('SUG_CHAMFER_MERGED', '1') != '0'  # A/B knob: 0 = one launch per direction (a -> b, b -> a)


def chamfer(a, b):
    """a [B,N,3], b [B,M,3] -> [B]: mean_i min_j d + mean_j min_i d."""
    _need_gpu(a, b)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    B, N, _ = a.shape
    M = b.shape[1]
    out = torch.empty(B, dtype=torch.float32, device=a.device)
    ws = torch.empty(lib().sug_chamfer_workspace(B, N, M), dtype=torch.float32, device=a.device)
    fn, name = (lib().sug_chamfer_merged, 'sug_chamfer_merged') if CHAMFER_MERGED else (lib().sug_chamfer, 'sug_chamfer')
    check(fn(_p(a), _p(b), B, N, M, _p(out), _p(ws), _st()), name)
    return out


def chamfer_weights(a, b, method):
    """distance2weights(chamfer(a, b), method) [B] for method in naive_inverse / exp_inverse / mean2one, the weighting inside
    the fold launch of the distance (sug_chamfer_weights)."""
    _need_gpu(a, b)
    if method not in ('naive_inverse', 'exp_inverse', 'mean2one'):
        raise RuntimeError('Not supported weighting method %s' % method)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    B, N, _ = a.shape
    M = b.shape[1]
    out = torch.empty(B, dtype=torch.float32, device=a.device)
    ws = torch.empty(lib().sug_chamfer_workspace(B, N, M), dtype=torch.float32, device=a.device)
    fn, name = (lib().sug_chamfer_weights_merged, 'sug_chamfer_weights_merged') if CHAMFER_MERGED else \
        (lib().sug_chamfer_weights, 'sug_chamfer_weights')
    check(fn(_p(a), _p(b), B, N, M, _SDA_METHODS[method], _p(out), _p(ws), _st()), name)
    return out


CHAMFER_MAX_POINTS = _H['SUG_CHAMFER_MAX_POINTS']


class _ChamferNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        B, N, _ = a.shape
        M = b.shape[1]
        dist1 = torch.empty(B, N, dtype=torch.float32, device=a.device)
        dist2 = torch.empty(B, M, dtype=torch.float32, device=a.device)
        idx1 = torch.empty(B, N, dtype=torch.int32, device=a.device)
        idx2 = torch.empty(B, M, dtype=torch.int32, device=a.device)
        check(lib().sug_chamfer_nn(_p(a), _p(b), B, N, M, _p(dist1), _p(dist2), _p(idx1), _p(idx2), _st()), 'sug_chamfer_nn')
        ctx.save_for_backward(a, b, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g1, g2, _gi1, _gi2):
        a, b, idx1, idx2 = ctx.saved_tensors
        B, N, _ = a.shape
        M = b.shape[1]
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None        # a side without a gradient: a null pointer
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        check(lib().sug_chamfer_nn_bwd(_p(g1.contiguous()), _p(g2.contiguous()), _p(a), _p(b), _p(idx1), _p(idx2), B, N, M,
                                       _p(ga), _p(gb), _st()), 'sug_chamfer_nn_bwd')
        return ga, gb


def chamfer_nn(a, b):
    """a [B,N,3], b [B,M,3] fp32 rows -> (dist1 [B,N], dist2 [B,M], idx1 [B,N], idx2 [B,M] int32): the squared distance of
    every point to its nearest neighbour in the other cloud and that neighbour's index (the lowest one on exact ties).
    dist1 / dist2 carry the gradient to both clouds (first order only; a point's terms are added in a fixed order, no
    atomics); the indices are not differentiable.  1 <= N, M <= CHAMFER_MAX_POINTS."""
    _need_gpu(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError('chamfer_nn: fp32 clouds only (got %s, %s)' % (a.dtype, b.dtype))
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3:
        raise RuntimeError('chamfer_nn: clouds are rows [B,N,3] and [B,M,3] (got %s, %s)' % (tuple(a.shape), tuple(b.shape)))
    if a.shape[0] != b.shape[0]:
        raise RuntimeError('chamfer_nn: %d clouds against %d: the clouds are paired' % (a.shape[0], b.shape[0]))
    return _ChamferNN.apply(a, b)


# ----------------------------------------------------------------------------- KPConv backbone
# Packed clouds (sug_amd/csrc/kpconv.hip, "ROW LAYOUT"): a level tensor has rows >= off[B] rows, of which the first off[B]
# are valid -- the clouds back to back at the int32 device offsets off [B+1] -- and the rest exactly zero, in and out;
# neighbour tables [Nq, H] int32 whose missing slots hold the shadow index Ns, the rows of the support tensor.  The valid
# counts are read on the device, so nothing here waits for the host.  Exact sizes are tensors of off[B] rows.
KPCONV_MAX_CLOUD = _H['SUG_KPCONV_MAX_CLOUD']          # the largest `cap` sug_grid_subsample / sug_radius_reverse take
KPCONV_RECORD_INTS = _H['SUG_KPCONV_RECORD_INTS']


def kp_grid_subsample(pts, off, B, cap, dl, rows=None, record=None, level=0):
    """Grid subsample of packed clouds pts [N,3] (offsets off, every cloud <= cap points) -> (packed voxel points
    [rows,3] (rows: N if None) of which the first sum-of-counts rows are valid and the others zero, their offsets [B+1]
    clamped to rows); with a `record` (int32 [KPCONV_RECORD_INTS]) the unclamped total goes into it at `level` (0 = the
    first pooled level).  Nothing is synchronised."""
    _need_gpu(pts, off, record)
    pts = pts.detach().contiguous()
    rows = pts.shape[0] if rows is None else rows
    pad = torch.empty(B, cap, 3, dtype=torch.float32, device=pts.device)
    cnt = torch.empty(B, dtype=torch.int32, device=pts.device)
    out = torch.empty(rows, 3, dtype=torch.float32, device=pts.device)
    out_off = torch.empty(B + 1, dtype=torch.int32, device=pts.device)
    check(lib().sug_grid_subsample(_p(pts), _p(off), B, cap, float(dl), rows, level, _p(pad), _p(cnt), _p(out), _p(out_off),
                                   _p(record), _st()), 'sug_grid_subsample')
    return out, out_off


def radius_neighbors(q, qoff, s, soff, radius, limit):
    """[Nq, limit] int32: per query the first `limit` supports of its cloud (support order) with d^2 < r^2, the shadow
    Ns = s.shape[0]; a dead query's row is all shadow."""
    _need_gpu(q, qoff, s, soff)
    q, s = q.detach().contiguous(), s.detach().contiguous()
    out = torch.empty(q.shape[0], limit, dtype=torch.int32, device=q.device)
    check(lib().sug_radius_neighbors(_p(q), _p(qoff), q.shape[0], _p(s), _p(soff), s.shape[0], qoff.numel() - 1,
                                     float(radius), limit, _p(out), _st()), 'sug_radius_neighbors')
    return out


def radius_reverse(nbr, qoff, soff, Ns, cap):
    """Sorted reverse lists of a neighbour table: (rev_be [Ns,2] with empty lists for the dead supports, rev_ent
    [Nq*H]); cap: no cloud has more supports (the level-0 cloud size will do: no cloud grows)."""
    _need_gpu(nbr, qoff, soff)
    Nq, H = nbr.shape
    be = torch.empty(Ns, 2, dtype=torch.int32, device=nbr.device)
    ent = torch.empty(max(1, Nq * H), dtype=torch.int32, device=nbr.device)
    check(lib().sug_radius_reverse(_p(nbr), _p(qoff), _p(soff), qoff.numel() - 1, H, Ns, cap, _p(be), _p(ent), _st()),
          'sug_radius_reverse')
    return be, ent


class _KPConvAgg(torch.autograd.Function):
    """wf [Nq, K*Cin]: the influence-weighted neighbour features of every kernel point, divided by the positive-row count
    (sug_kpconv_fwd); backward dx through the support's reverse lists (sug_kpconv_bwd).  qoff's last entry is the number
    of valid queries (read on the device)."""

    @staticmethod
    def forward(ctx, x, q, s, nbr, kp, extent, rev, qoff):
        _need_gpu(x, q, s, nbr, kp, qoff)
        x = x.contiguous()
        Nq, H = nbr.shape
        K, Cin = kp.shape[0], x.shape[1]
        wf = torch.empty(Nq, K * Cin, dtype=torch.float32, device=x.device)
        w = torch.empty(Nq, H, K, dtype=torch.float32, device=x.device)
        cnt = torch.empty(Nq, dtype=torch.float32, device=x.device)
        check(_timed('kpconv_fwd', {'Nq': Nq, 'Cin': Cin},
                     lambda: lib().sug_kpconv_fwd(_p(q), _p(s), _p(nbr), _p(qoff[-1:]), Nq, H, s.shape[0],
                                                  _p(kp.detach().contiguous()), K, float(extent), _p(x), Cin, _p(wf),
                                                  _p(w), _p(cnt), _st())), 'sug_kpconv_fwd')
        ctx.save_for_backward(w, cnt)
        ctx.rev, ctx.dims = rev, (H, K, s.shape[0], Cin)
        return wf

    @staticmethod
    def backward(ctx, g):
        w, cnt = ctx.saved_tensors
        H, K, Ns, Cin = ctx.dims
        g = g.contiguous()
        dx = torch.empty(Ns, Cin, dtype=torch.float32, device=g.device)
        be, ent = ctx.rev
        check(_timed('kpconv_bwd', {'Ns': Ns, 'Cin': Cin},
                     lambda: lib().sug_kpconv_bwd(_p(be), _p(ent), H, K, _p(w), _p(cnt), _p(g), Ns, Cin, _p(dx), _st())),
              'sug_kpconv_bwd')
        return dx, None, None, None, None, None, None, None


def kpconv(x, q, s, nbr, rev, kernel_points, weights, extent, qoff):
    """KPConv (rigid, linear influence, sum): [Nq, Cout] = (wf / count) . W with W [K, Cin, Cout] viewed as [K*Cin, Cout];
    rev = radius_reverse(nbr, ...), qoff the query level's offsets.  The GEMM runs on all Nq rows, the dead ones being
    zero."""
    _need_gpu(x, q, s, nbr, kernel_points, weights)
    K, Cin, Cout = weights.shape
    wf = _KPConvAgg.apply(x, q, s, nbr, kernel_points, extent, rev, qoff)
    return linear_rows(wf, weights.view(K * Cin, Cout).t())


class _SegInstNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, off, mode, sc):
        _need_gpu(x, off, sc)
        x = x.contiguous()
        B, (N, C) = off.numel() - 1, x.shape
        y = torch.empty_like(x)
        mean = torch.empty(B, C, dtype=torch.float32, device=x.device)
        rstd = torch.empty(B, C, dtype=torch.float32, device=x.device)
        scc = sc.contiguous() if sc is not None else None
        check(lib().sug_seg_instnorm_fwd(_p(x), _p(off), B, N, C, 1e-5, mode, _p(scc), _p(y), _p(mean), _p(rstd), _st()),
              'sug_seg_instnorm_fwd')
        ctx.save_for_backward(x, y, mean, rstd, off)
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, mean, rstd, off = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(x)
        dsc = torch.empty_like(x) if ctx.mode == 2 else None
        check(lib().sug_seg_instnorm_bwd(_p(g), _p(y), _p(x), _p(mean), _p(rstd), _p(off), off.numel() - 1, x.shape[0],
                                         x.shape[1], ctx.mode, _p(dx), _p(dsc), _st()), 'sug_seg_instnorm_bwd')
        return dx, None, None, dsc


def seg_instnorm(x, off, act=False, shortcut=None):
    """Per-cloud InstanceNorm1d of rows x [N, C] (clouds at offsets off), then LeakyReLU(0.1) if act; with a shortcut
    [N, C]: LeakyReLU(0.1)(norm(x) + shortcut).  The dead rows [off[B], N) of the result and of the gradients are zero.
    An empty cloud normalises nothing (it used to divide by zero where x had exactly off[B] rows)."""
    mode = 2 if shortcut is not None else (1 if act else 0)
    return _SegInstNorm.apply(x, off, mode, shortcut)


class _SegMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nbr, rev):
        _need_gpu(x, nbr)
        x = x.contiguous()
        Nq, H = nbr.shape
        Ns, C = x.shape
        y = torch.empty(Nq, C, dtype=torch.float32, device=x.device)
        arg = torch.empty(Nq, C, dtype=torch.int32, device=x.device)
        check(lib().sug_seg_max_pool_fwd(_p(x), _p(nbr), Nq, H, Ns, C, _p(y), _p(arg), _st()), 'sug_seg_max_pool_fwd')
        ctx.save_for_backward(arg)
        ctx.rev, ctx.dims = rev, (H, Ns, C)
        return y

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        H, Ns, C = ctx.dims
        g = g.contiguous()
        dx = torch.empty(Ns, C, dtype=torch.float32, device=g.device)
        be, ent = ctx.rev
        check(lib().sug_seg_max_pool_bwd(_p(g), _p(arg), _p(be), _p(ent), H, Ns, C, _p(dx), _st()), 'sug_seg_max_pool_bwd')
        return dx, None, None


def seg_max_pool(x, nbr, rev):
    """[Nq, C]: max over each query's slots of x rows, a shadow slot reading 0 (model/KPConv_blocks.py max_pool)."""
    return _SegMaxPool.apply(x, nbr, rev)


class _SegMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, off):
        _need_gpu(x, off)
        x = x.contiguous()
        B, C = off.numel() - 1, x.shape[1]
        y = torch.empty(B, C, dtype=torch.float32, device=x.device)
        check(lib().sug_seg_mean_fwd(_p(x), _p(off), B, C, _p(y), _st()), 'sug_seg_mean_fwd')
        ctx.save_for_backward(off)
        ctx.N = x.shape[0]
        return y

    @staticmethod
    def backward(ctx, g):
        (off,) = ctx.saved_tensors
        g = g.contiguous()
        B, C = g.shape
        dx = torch.empty(ctx.N, C, dtype=torch.float32, device=g.device)
        check(lib().sug_seg_mean_bwd(_p(g), _p(off), B, ctx.N, C, _p(dx), _st()), 'sug_seg_mean_bwd')
        return dx, None


def seg_mean(x, off):
    """[B, C]: per-cloud mean of the rows x [N, C] (model/KPConv_model.py global_average).  An empty cloud's row is zero,
    with a zero gradient (it used to be NaN where x had exactly off[B] rows)."""
    return _SegMean.apply(x, off)


def kp_sample_rows(x, off, sampled_len=64):
    """[B, sampled_len, D]: sample_tensor_slices of the rows x [C_l, D] from the device offsets off [B+1] (forward only:
    the reference detaches this tensor)."""
    _need_gpu(x, off)
    x = x.detach().contiguous()
    B, D = off.numel() - 1, x.shape[1]
    out = torch.empty(B, sampled_len, D, dtype=torch.float32, device=x.device)
    check(lib().sug_kp_sample_rows(_p(x), _p(off), B, sampled_len, D, _p(out), _st()), 'sug_kp_sample_rows')
    return out


# ----------------------------------------------------------------------------- data pipeline
PREP_NORMALIZE, PREP_ROTATE_Z, PREP_JITTER, PREP_SHUFFLE, PREP_MAX_POINTS = (          # the stage bits and the limit on P
    _H['SUG_PREP_' + _n] for _n in ('NORMALIZE', 'ROTATE_Z', 'JITTER', 'SHUFFLE', 'MAX_POINTS'))


def rotation_matrix(axis, angle):
    """rotate_shape's matrix (data/data_utils.py:47-49) for `x.dot(R)`, evaluated in fp64, as 9 floats row-major."""
    c, s = math.cos(angle), math.sin(angle)
    if axis == 'x':
        return (1.0, 0.0, 0.0, 0.0, c, -s, 0.0, s, c)
    if axis == 'y':
        return (c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c)
    return (c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0)


_PRE_ROTATE_X = rotation_matrix('x', -math.pi / 2)              # UnifiedPointDG's fixed pre-rotation


def prepare_batch(pts, idx, num_points, pre_rotate, aug, *, angles=None, noise=None, sel=None, seed=None, counter=None,
                  out=None, sigma=0.01, clip=0.05, return_draws=False, stages=None, pre_matrix=None):
    """UnifiedPointDG.__getitem__ for a batch in one launch (sug_prepare_batch): pts [M,P,3] fp32 resident dataset,
    idx [B] int32 -> [B,3,num_points] fp32.  Random inputs come from `angles` [B] / `noise` [B,P,3] / `sel` [B,N] when
    given, else from the in-kernel Philox generator keyed by `seed` at the batch counter held in the device tensor
    `counter` (int64, one element).  `stages` overrides the stage bits (default: normalise, plus z-rotation and jitter when
    `aug`), `pre_matrix` (9 floats) the pre-rotation (default rotate_shape(.., 'x', -pi/2) when `pre_rotate`).
    return_draws: also (angles [B], noise [B,N,3] per kept point, sel [B,N]).  No host synchronisation; with `out` and
    `counter` given the call is one kernel launch and can be captured."""
    _need_gpu(pts, idx, angles, noise, sel, counter, out)
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float32 or not pts.is_contiguous():
        raise ValueError('prepare_batch: pts must be a contiguous fp32 [M, P, 3] tensor, got %s %s' % (tuple(pts.shape), pts.dtype))
    if idx.dim() != 1 or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise ValueError('prepare_batch: idx must be a contiguous int32 [B] tensor')
    M, P, _ = pts.shape
    B, N = idx.shape[0], int(num_points)
    dev = pts.device
    if stages is None:
        stages = PREP_NORMALIZE | ((PREP_ROTATE_Z | PREP_JITTER) if aug else 0)
    if pre_matrix is None and pre_rotate:
        pre_matrix = _PRE_ROTATE_X
    pre = (ctypes.c_float * 9)(*pre_matrix) if pre_matrix is not None else None

    def given(t, shape, dtype, name):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()):
            raise ValueError('prepare_batch: %s must be a contiguous %s tensor of shape %s, got %s %s'
                             % (name, dtype, shape, t.dtype, tuple(t.shape)))
    given(angles, (B,), torch.float32, 'angles')
    given(noise, (B, P, 3), torch.float32, 'noise')
    given(sel, (B, N), torch.int32, 'sel')
    given(out, (B, 3, N), torch.float32, 'out')
    given(counter, (1,), torch.int64, 'counter')
    if out is None:
        out = torch.empty(B, 3, N, dtype=torch.float32, device=dev)
    a_out = n_out = s_out = None
    if return_draws:
        a_out = torch.empty(B, dtype=torch.float32, device=dev)
        n_out = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        s_out = torch.empty(B, N, dtype=torch.int32, device=dev)
    seed = 0 if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    check(lib().sug_prepare_batch(_p(pts), M, P, _p(idx), B, N, stages, pre, _p(angles), _p(noise), _p(sel), seed,
                                  _p(counter), sigma, clip, _p(out), _p(a_out), _p(n_out), _p(s_out), _st()),
          'sug_prepare_batch')
    return (out, a_out, n_out, s_out) if return_draws else out


PREP_SCALE, PREP_PERTURB, PREP_SHIFT, PREP_AUG_PARAMS = (                               # sug_prepare_batch_aug's extra stages
    _H['SUG_PREP_' + _n] for _n in ('SCALE', 'PERTURB', 'SHIFT', 'AUG_PARAMS'))
_PREP_AUG_SLOTS = tuple(_H['SUG_PREP_AUG_' + _n] for _n in ('SCALE_LOW', 'SCALE_HIGH', 'SHIFT_RANGE', 'ANGLE_SIGMA', 'ANGLE_CLIP'))


def prepare_batch_aug(pts, idx, num_points, pre_rotate, aug, *, angles=None, noise=None, sel=None, scales=None, perturb=None,
                      shifts=None, seed=None, counter=None, out=None, sigma=0.01, clip=0.05, scale_low=0.8, scale_high=1.25,
                      shift_range=0.1, angle_sigma=0.06, angle_clip=0.18, return_draws=False, stages=None, pre_matrix=None):
    """prepare_batch with the scale, rotation-perturbation and shift stages (sug_prepare_batch_aug), applied behind the
    jitter in pc_augment's line order.  `stages` selects the stage bits (default: prepare_batch's, i.e. none of the three
    new ones; add PREP_SCALE | PREP_PERTURB | PREP_SHIFT).  The per-cloud draws come from `scales` [B] (the factor),
    `perturb` [B,3] (standard normals, scaled by angle_sigma and clipped to +-angle_clip in the kernel) and `shifts` [B,3]
    (the vector) when given, else from the in-kernel generator at (`seed`, `counter`).  return_draws: (out, angles [B],
    noise [B,N,3], sel [B,N], scales [B], perturb [B,3], shifts [B,3]).  No host synchronisation; with `out` and `counter`
    given the call is one kernel launch and can be captured."""
    _need_gpu(pts, idx, angles, noise, sel, scales, perturb, shifts, counter, out)
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float32 or not pts.is_contiguous():
        raise ValueError('prepare_batch_aug: pts must be a contiguous fp32 [M, P, 3] tensor, got %s %s' % (tuple(pts.shape), pts.dtype))
    if idx.dim() != 1 or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise ValueError('prepare_batch_aug: idx must be a contiguous int32 [B] tensor')
    M, P, _ = pts.shape
    B, N = idx.shape[0], int(num_points)
    dev = pts.device
    if stages is None:
        stages = PREP_NORMALIZE | ((PREP_ROTATE_Z | PREP_JITTER) if aug else 0)
    if pre_matrix is None and pre_rotate:
        pre_matrix = _PRE_ROTATE_X
    pre = (ctypes.c_float * 9)(*pre_matrix) if pre_matrix is not None else None
    params = (ctypes.c_float * PREP_AUG_PARAMS)()
    for slot, v in zip(_PREP_AUG_SLOTS, (scale_low, scale_high, shift_range, angle_sigma, angle_clip)):
        params[slot] = v

    def given(t, shape, dtype, name):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()):
            raise ValueError('prepare_batch_aug: %s must be a contiguous %s tensor of shape %s, got %s %s'
                             % (name, dtype, shape, t.dtype, tuple(t.shape)))
    given(angles, (B,), torch.float32, 'angles')
    given(noise, (B, P, 3), torch.float32, 'noise')
    given(sel, (B, N), torch.int32, 'sel')
    given(scales, (B,), torch.float32, 'scales')
    given(perturb, (B, 3), torch.float32, 'perturb')
    given(shifts, (B, 3), torch.float32, 'shifts')
    given(out, (B, 3, N), torch.float32, 'out')
    given(counter, (1,), torch.int64, 'counter')
    if out is None:
        out = torch.empty(B, 3, N, dtype=torch.float32, device=dev)
    draws = [None] * 6
    if return_draws:
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        draws = [f32(B), f32(B, N, 3), torch.empty(B, N, dtype=torch.int32, device=dev), f32(B), f32(B, 3), f32(B, 3)]
    seed = 0 if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    check(lib().sug_prepare_batch_aug(_p(pts), M, P, _p(idx), B, N, stages, pre, _p(angles), _p(noise), _p(sel), _p(scales),
                                      _p(perturb), _p(shifts), seed, _p(counter), sigma, clip, params, _p(out),
                                      *[_p(d) for d in draws], _st()), 'sug_prepare_batch_aug')
    return (out, *draws) if return_draws else out


PREP_NORMALS, PREP_SEG_MAX_EXTRA = _H['SUG_PREP_NORMALS'], _H['SUG_PREP_SEG_MAX_EXTRA']   # sug_prepare_seg_batch


def prepare_seg_batch(pts, extra, point_label, category, lengths, idx, num_points, *, angles=None, noise=None, sel=None,
                      scales=None, perturb=None, shifts=None, seed=None, counter=None, out=None, label_out=None,
                      category_out=None, sigma=0.01, clip=0.05, scale_low=0.8, scale_high=1.25, shift_range=0.1,
                      angle_sigma=0.06, angle_clip=0.18, return_draws=False, stages=None, pre_matrix=None):
    """The part-segmentation batch in one launch (sug_prepare_seg_batch): pts [M,P,3] fp32, extra [M,P,E] fp32 or None,
    point_label [M,P] uint8, category [M] int64, lengths [M] int32 or None (every cloud has P points), idx [B] int32 ->
    (points [B,3+E,num_points] fp32, category [B] int64, label [B,num_points] int64), the argument order of SegStep.step.
    Every output row is a real point: a cloud longer than num_points gives a random ordered subset, a shorter one all its
    points and then draws with replacement.  `stages` (default PREP_NORMALIZE) selects prepare_batch_aug's stage bits and
    PREP_NORMALS, which turns extra channels 0..2 with the cloud; the draws come from the keywords when given (`sel` may
    repeat points), else from the in-kernel generator at (`seed`, `counter`).  return_draws: the three outputs, then
    prepare_batch_aug's draws, with sel [B,N] the source point of every row.  No host synchronisation; with `out`,
    `label_out`, `category_out` and `counter` given the call is one kernel launch and can be captured."""
    _need_gpu(pts, extra, point_label, category, lengths, idx, angles, noise, sel, scales, perturb, shifts, counter, out,
              label_out, category_out)
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float32 or not pts.is_contiguous():
        raise ValueError('prepare_seg_batch: pts must be a contiguous fp32 [M, P, 3] tensor, got %s %s' % (tuple(pts.shape), pts.dtype))
    if idx.dim() != 1 or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise ValueError('prepare_seg_batch: idx must be a contiguous int32 [B] tensor')
    M, P, _ = pts.shape
    B, N = idx.shape[0], int(num_points)
    dev = pts.device
    if extra is not None and (extra.dim() != 3 or tuple(extra.shape[:2]) != (M, P)):
        raise ValueError('prepare_seg_batch: extra must be [M, P, E] = [%d, %d, E], got %s' % (M, P, tuple(extra.shape)))
    E = 0 if extra is None else int(extra.shape[2])
    if E == 0:
        extra = None
    if stages is None:
        stages = PREP_NORMALIZE
    pre = (ctypes.c_float * 9)(*pre_matrix) if pre_matrix is not None else None
    params = (ctypes.c_float * PREP_AUG_PARAMS)()
    for slot, v in zip(_PREP_AUG_SLOTS, (scale_low, scale_high, shift_range, angle_sigma, angle_clip)):
        params[slot] = v

    def given(t, shape, dtype, name):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()):
            raise ValueError('prepare_seg_batch: %s must be a contiguous %s tensor of shape %s, got %s %s'
                             % (name, dtype, shape, t.dtype, tuple(t.shape)))
    if point_label is None or category is None:
        raise ValueError('prepare_seg_batch: point_label [M, P] uint8 and category [M] int64 are required')
    given(extra, (M, P, E), torch.float32, 'extra')
    given(point_label, (M, P), torch.uint8, 'point_label')
    given(category, (M,), torch.int64, 'category')
    given(lengths, (M,), torch.int32, 'lengths')
    given(angles, (B,), torch.float32, 'angles')
    given(noise, (B, P, 3), torch.float32, 'noise')
    given(sel, (B, N), torch.int32, 'sel')
    given(scales, (B,), torch.float32, 'scales')
    given(perturb, (B, 3), torch.float32, 'perturb')
    given(shifts, (B, 3), torch.float32, 'shifts')
    given(out, (B, 3 + E, N), torch.float32, 'out')
    given(label_out, (B, N), torch.int64, 'label_out')
    given(category_out, (B,), torch.int64, 'category_out')
    given(counter, (1,), torch.int64, 'counter')
    if out is None:
        out = torch.empty(B, 3 + E, N, dtype=torch.float32, device=dev)
    if label_out is None:
        label_out = torch.empty(B, N, dtype=torch.int64, device=dev)
    if category_out is None:
        category_out = torch.empty(B, dtype=torch.int64, device=dev)
    draws = [None] * 6
    if return_draws:
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        draws = [f32(B), f32(B, N, 3), torch.empty(B, N, dtype=torch.int32, device=dev), f32(B), f32(B, 3), f32(B, 3)]
    seed = 0 if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    check(lib().sug_prepare_seg_batch(_p(pts), _p(extra), _p(point_label), _p(category), _p(lengths), M, P, E, _p(idx), B, N,
                                      stages, pre, _p(angles), _p(noise), _p(sel), _p(scales), _p(perturb), _p(shifts), seed,
                                      _p(counter), sigma, clip, params, _p(out), _p(label_out), _p(category_out),
                                      *[_p(d) for d in draws], _st()), 'sug_prepare_seg_batch')
    return (out, category_out, label_out, *draws) if return_draws else (out, category_out, label_out)


# ----------------------------------------------------------------------------- sub-domain splitter
ICP_MAX_POINTS = _H['SUG_ICP_MAX_POINTS']


def icp_fitness(src, tgt, max_corr_dist=0.15, max_iteration=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """Point-to-point ICP of B (source, target) pairs in one launch (sug_icp_fitness; open3d's registration_icp with its
    defaults, restated in include/sug_amd.h): src [Ns, 3] (one source for every pair) or [B, Ns, 3], tgt [B, Nt, 3], fp32
    -> (count int32 [B], rmse fp64 [B], iters int32 [B], transform fp64 [B, 4, 4]); fitness = count / Ns.  No host
    synchronisation."""
    _need_gpu(src, tgt)
    if tgt.dim() != 3 or tgt.shape[2] != 3 or src.dim() not in (2, 3) or src.shape[-1] != 3:
        raise ValueError('icp_fitness: src must be [Ns, 3] or [B, Ns, 3] and tgt [B, Nt, 3], got %s and %s'
                         % (tuple(src.shape), tuple(tgt.shape)))
    if src.dtype != torch.float32 or tgt.dtype != torch.float32:
        raise ValueError('icp_fitness: fp32 clouds only, got %s and %s' % (src.dtype, tgt.dtype))
    B, Nt, _ = tgt.shape
    if src.dim() == 3 and src.shape[0] != B:
        raise ValueError('icp_fitness: %d sources for %d targets' % (src.shape[0], B))
    src, tgt = src.detach().contiguous(), tgt.detach().contiguous()
    Ns = src.shape[-2]
    stride = 0 if src.dim() == 2 else 3 * Ns
    dev = tgt.device
    count = torch.empty(B, dtype=torch.int32, device=dev)
    rmse = torch.empty(B, dtype=torch.float64, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    transform = torch.empty(B, 4, 4, dtype=torch.float64, device=dev)
    check(_timed('icp_fitness', {'B': B, 'Ns': Ns, 'Nt': Nt},
                 lambda: lib().sug_icp_fitness(_p(src), stride, _p(tgt), B, Ns, Nt, float(max_corr_dist), int(max_iteration),
                                               float(rel_fitness), float(rel_rmse), _p(count), _p(rmse), _p(iters),
                                               _p(transform), _st())), 'sug_icp_fitness')
    return count, rmse, iters, transform


PFH_MAX_POINTS = _H['SUG_PFH_MAX_POINTS']
PFH_MAX_NEIGHBORS = _H['SUG_PFH_MAX_NEIGHBORS']


def pfh_descriptors(pts, rad=0.2, nneighbors=8, div=2):
    """Point Feature Histograms of M clouds in one launch (sug_pfh_descriptors; PFH.calc_normals and PFH.calcHistArray of
    utils/pfh.py, restated in include/sug_amd.h): pts [M, N, 3] fp32 -> (hist fp64 [M, N, div^3], normals fp64 [M, N, 3],
    nbr_idx int32 [M, N, k] padded with -1, nbr_cnt int32 [M, N], used_cnt int32 [M]).  A point without a neighbour inside
    `rad` is unused: a zero row, nbr_cnt 0.  No host synchronisation."""
    _need_gpu(pts)
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise ValueError('pfh_descriptors: pts must be [M, N, 3], got %s' % (tuple(pts.shape),))
    if pts.dtype != torch.float32:
        raise ValueError('pfh_descriptors: fp32 clouds only, got %s' % pts.dtype)
    M, N, _ = pts.shape
    k, div = int(nneighbors), int(div)
    if not 1 <= k <= PFH_MAX_NEIGHBORS or not 2 <= div <= 5:
        raise ValueError('pfh_descriptors: nneighbors=%d outside 1 .. %d or div=%d outside 2 .. 5' % (k, PFH_MAX_NEIGHBORS, div))
    pts = pts.detach().contiguous()
    dev = pts.device
    hist = torch.empty(M, N, div ** 3, dtype=torch.float64, device=dev)
    normals = torch.empty(M, N, 3, dtype=torch.float64, device=dev)
    nbr_idx = torch.empty(M, N, k, dtype=torch.int32, device=dev)
    nbr_cnt = torch.empty(M, N, dtype=torch.int32, device=dev)
    used_cnt = torch.empty(M, dtype=torch.int32, device=dev)
    check(_timed('pfh_descriptors', {'M': M, 'N': N, 'k': k, 'div': div},
                 lambda: lib().sug_pfh_descriptors(_p(pts), M, N, float(rad), k, div, _p(hist), _p(normals), _p(nbr_idx),
                                                   _p(nbr_cnt), _p(used_cnt), _st())), 'sug_pfh_descriptors')
    return hist, normals, nbr_idx, nbr_cnt, used_cnt


def pfh_hist_distance(histS, cntS, histT, cntT):
    """pfh_hist_distance of utils/pfh.py:146-159 for B (source, target) descriptor sets in one launch
    (sug_pfh_hist_distance): histS [Ns, D] with cntS [Ns] (one source for every pair) or [B, Ns, D] with [B, Ns]; histT
    [B, Nt, D], cntT [B, Nt]; fp64 histograms, int32 neighbour counts (a row is used iff its count is > 0) -> fp64 [B]: the
    median over the used source rows of the distance to the nearest used target row, NaN when either side has none.  No
    host synchronisation."""
    _need_gpu(histS, cntS, histT, cntT)
    if histT.dim() != 3 or histS.dim() not in (2, 3) or histS.shape[-1] != histT.shape[-1]:
        raise ValueError('pfh_hist_distance: histS must be [Ns, D] or [B, Ns, D] and histT [B, Nt, D], got %s and %s'
                         % (tuple(histS.shape), tuple(histT.shape)))
    if tuple(cntS.shape) != tuple(histS.shape[:-1]) or tuple(cntT.shape) != tuple(histT.shape[:-1]):
        raise ValueError('pfh_hist_distance: counts %s and %s do not match the histograms %s and %s'
                         % (tuple(cntS.shape), tuple(cntT.shape), tuple(histS.shape), tuple(histT.shape)))
    if histS.dtype != torch.float64 or histT.dtype != torch.float64 or cntS.dtype != torch.int32 or cntT.dtype != torch.int32:
        raise ValueError('pfh_hist_distance: fp64 histograms and int32 counts only, got %s, %s, %s, %s'
                         % (histS.dtype, histT.dtype, cntS.dtype, cntT.dtype))
    B, Nt, D = histT.shape
    if histS.dim() == 3 and histS.shape[0] != B:
        raise ValueError('pfh_hist_distance: %d sources for %d targets' % (histS.shape[0], B))
    histS, cntS, histT, cntT = (x.detach().contiguous() for x in (histS, cntS, histT, cntT))
    Ns = histS.shape[-2]
    stride = 0 if histS.dim() == 2 else Ns * D
    out = torch.empty(B, dtype=torch.float64, device=histT.device)
    check(_timed('pfh_hist_distance', {'B': B, 'Ns': Ns, 'Nt': Nt, 'D': D},
                 lambda: lib().sug_pfh_hist_distance(_p(histS), _p(cntS), stride, _p(histT), _p(cntT), B, Ns, Nt, D, _p(out),
                                                     _st())), 'sug_pfh_hist_distance')
    return out


def _ctx_property(field):
    return property(lambda self: getattr(CTX, field), lambda self, v: setattr(CTX, field, v))


class _OpsModule(type(_os)):
    """The old module-level names of the context fields: `ops.BN_GROUPS`, `ops.START_PROVIDER = f`, ... read and write CTX
    (see StepContext)."""
    BN_GROUPS = _ctx_property('bn_groups')
    START_QUEUE = _ctx_property('start_queue')
    START_PROVIDER = _ctx_property('start_provider')
    GEOMETRY_PLAN = _ctx_property('geometry_plan')
    PROFILE_ONLY = _ctx_property('profile_only')
    PROFILE = _ctx_property('profile')
    PARALLEL_BRANCHES = _ctx_property('parallel_branches')
    FUSED_HEADS = _ctx_property('fused_heads')
    W16_CACHE = _ctx_property('w16_cache')
    BN_RECORD = _ctx_property('bn_record')
    _PENDING_COUNTS = _ctx_property('pending_counts')


import sys as _sys
_sys.modules[__name__].__class__ = _OpsModule
