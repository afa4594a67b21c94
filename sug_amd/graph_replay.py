"""What the hipGraph front ends share: the three that replay a forward or SUGStep's own step (SUGStep's graph step,
call_graphs.CallGraphs, eval_graphs.EvalRunner) and the step classes built on `ReplayedStep` (SourceStep, UDAStep).

Each of them runs a key eagerly once under `StartFeeder.recording()`, captures it under `StartFeeder.providing()` and from
then on copies the inputs, calls `refill()` and replays.  The capture itself stays written out at each site, as
`with feeder.providing(), ops.capture_guard(), torch.cuda.graph(...)`; no context manager is entered and nothing new is
allocated on a replay path.  The small choices every step class makes the same way (Adam class, by-value hyper key, plan
generations, weight caches, the plain-CE predicate) are the functions at the end.
"""
import collections
import contextlib

import torch
import torch.nn as nn

from . import ops


class StartFeeder:
    """FPS start indices for a replayable forward / step: drawn from the CPU default generator in call
    order with the same (B, N) sequence as an eager run (so the random stream is the
    reference's, model/point_utils.py:17), but delivered through one static device buffer."""

    def __init__(self, device):
        self.device = device
        self.plan = []          # (B, N) per farthest_point_sample call
        self.host = self.dev = None
        self.cursor = 0

    def record(self, B, N):     # provider during the eager planning run
        self.plan.append((B, N))
        return torch.randint(0, N, (B,), dtype=torch.long)

    def recording(self):
        """The eager planning run: every draw inside the block is made as usual and its (B, N) noted in `plan`."""
        return ops.CTX.scoped(start_provider=self.record)

    def build(self):
        total = max(sum(b for b, _ in self.plan), 1)
        # two pinned staging buffers, used alternately: the host must not overwrite one while its
        # asynchronous copy to the device may still be pending (replays are not synchronised)
        self.host = [torch.empty(total, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.done = [None, None]
        self.turn = 0
        self.dev = torch.zeros(total, dtype=torch.int32, device=self.device)

    def refill(self):           # before every replay
        if not self.plan:
            return
        h = self.host[self.turn]
        if self.done[self.turn] is not None:
            self.done[self.turn].synchronize()
        off = 0
        for B, N in self.plan:
            h[off:off + B] = torch.randint(0, N, (B,), dtype=torch.long).to(torch.int32)
            off += B
        self.dev.copy_(h, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.done[self.turn] = ev
        self.turn ^= 1

    def provide(self, B, N):    # provider during capture
        off = sum(b for b, _ in self.plan[:self.cursor])
        assert self.cursor < len(self.plan) and self.plan[self.cursor] == (B, N), \
            'forward structure changed between planning and capture'
        self.cursor += 1
        return self.dev[off:off + B]

    @contextlib.contextmanager
    def providing(self):
        """The capture: the draws of the block are slices of the static buffer, in plan order.  A block that ends without
        an exception must have taken every planned draw -- one fewer would shift every later start of every replay."""
        self.cursor = 0
        with ops.CTX.scoped(start_provider=self.provide):
            yield
        if self.cursor != len(self.plan):
            raise RuntimeError('the captured forward drew %d FPS starts, the eager one %d' % (self.cursor, len(self.plan)))


class LRU(collections.OrderedDict):
    """An OrderedDict bounded to `limit` entries: get() marks an entry used, put() evicts the least recently used ones."""

    def __init__(self, limit, on_evict=None):
        super().__init__()
        self.limit, self.on_evict = limit, on_evict

    def get(self, k, default=None):
        if k in self:
            self.move_to_end(k)
            return self[k]
        return default

    def put(self, k, v):
        self[k] = v
        self.move_to_end(k)
        while len(self) > self.limit:
            _, old = self.popitem(last=False)
            if self.on_evict is not None:
                self.on_evict(old)
        return v


def refusal_text(exc):
    """The reason recorded for a refused capture: exception type and the first line of its message."""
    return '%s: %s' % (type(exc).__name__, str(exc).splitlines()[0] if str(exc) else '')


def tensor_outputs(out):
    """(outs, single): one tensor or a tuple of tensors (or None) as a list, and whether it was the single tensor."""
    single = isinstance(out, torch.Tensor)
    return ([out] if single else list(out if out is not None else ())), single


def adam_choice(on_gpu, fused_adam, use_graph):
    """(Adam class, keyword arguments).  fused_adam None/True -> sug_amd.optim.Adam (one launch per optimizer) on a HIP
    device, with step count / bias corrections / lr on the device; False, or a CPU -> torch.optim.Adam, capturable under
    `use_graph` only."""
    if on_gpu and (fused_adam is None or fused_adam):
        from .optim import Adam
        return Adam, {'graph_capturable': True}
    return torch.optim.Adam, ({'capturable': True, 'fused': True} if use_graph else {})


def hyper_key(opt):
    """What a captured step bakes in of an optimizer by value.  sug_amd.optim.Adam keeps lr on the device (one graph serves
    a whole schedule); any other optimizer takes it by value, so there the lr of every group is part of the key."""
    if hasattr(opt, 'graph_key'):
        return opt.graph_key()
    return tuple((g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) for g in opt.param_groups)


def plan_generations(opts):
    """The device-side plan generation of every optimizer-like object (0 for one without, None included): a captured graph
    holds raw pointers into those plans and must not outlive them."""
    return tuple(getattr(o, 'plan_generation', 0) for o in opts)


def drop_weight_caches(model, split_layers, prefix):
    """Nothing computed from the weights outlives the update that follows: the encoder's prefix cache (if `prefix`) and the
    EdgeConv weight-split cache of every layer in `split_layers`."""
    if prefix:
        model.g.clear_prefix_cache()
    for m in split_layers:
        m._wcat = None


def plain_ce(criterion, smoothing_ok=False):
    """A criterion the fused CE kernels compute exactly: nn.CrossEntropyLoss itself, no class weights, reduction 'mean' and --
    unless the caller's kernel takes it (`smoothing_ok`) -- no label smoothing."""
    c = criterion
    return type(c) is nn.CrossEntropyLoss and c.weight is None and c.reduction == 'mean' and \
        (smoothing_ok or c.label_smoothing == 0.0)


FusedCriterion = collections.namedtuple('FusedCriterion', 'kind alpha gamma reduction ignore_index')


def fused_criterion(criterion, C):
    """None, or what ops.cls_loss needs to compute `criterion` on C classes, by value: (kind, alpha as a host tuple | None, gamma,
    reduction, ignore_index).  Recognised: a plain nn.CrossEntropyLoss (kind 'ce') and an object whose type is exactly
    model_utils.focal_loss (kind 'focal': CLS_LOSS FocalLoss, and ClassWeighting = gamma 0) with a 1-D alpha of at least C
    entries, on either device, and gamma == 0 or gamma >= 1.  Reading a device alpha waits for the device: the steps ask through a
    CriterionState, which reads it again only when the tensor was replaced or written to."""
    from .model.model_utils import focal_loss
    c = criterion
    if plain_ce(c):
        return FusedCriterion('ce', None, 0.0, 'mean', int(c.ignore_index))
    if type(c) is not focal_loss:
        return None
    a, gamma = getattr(c, 'alpha', None), getattr(c, 'gamma', None)
    if not isinstance(a, torch.Tensor) or a.dim() != 1 or a.numel() < C or not a.is_floating_point():
        return None
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not (gamma == 0 or 1 <= gamma < float('inf')):
        return None
    alpha = tuple(a.detach().to(dtype=torch.float32).tolist())
    return FusedCriterion('focal', alpha, float(gamma), 'mean' if c.size_average else 'sum', -100)


class CriterionState:
    """A step's view of its criterion: the FusedCriterion record of the criterion as it is NOW (a host compare per step: the alpha
    tensor's identity and version, gamma, size_average; the record is formed again when one of them changed) and, per record, a
    device copy of alpha that belongs to the step.  A record is part of the step's graph key, and a captured step holds the raw
    pointer of its record's copy: the copies are kept least recently used first out, `limit` >= the number of captured steps
    kept and every step touches its record, so a copy outlives every graph captured with it."""

    def __init__(self, limit=4):
        self.limit = int(limit)
        self._seen = self._record = None
        self._dev = LRU(self.limit)

    def record(self, criterion, limit=None):
        c = criterion
        if type(c) is nn.CrossEntropyLoss:                  # (no failing attribute look-ups on a Module: this runs every step)
            a, seen = None, (c, c.ignore_index, c.weight is None, c.reduction, c.label_smoothing)
        else:
            a = getattr(c, 'alpha', None)
            seen = (c, type(c), getattr(a, '_version', None), getattr(c, 'gamma', None), getattr(c, 'size_average', None))
        if self._seen is None or self._seen[1] is not a or self._seen[0] != seen:
            self._seen, self._record = (seen, a), fused_criterion(c, 0)
        if limit is not None:
            self._dev.limit = self.limit = max(int(limit), 1)
        if self._record is not None and self._record in self._dev:
            self._dev.move_to_end(self._record)
        return self._record

    def alpha_on(self, record, device):
        """The device copy of record.alpha (None for a record without).  A new record is uploaded here, which is why the first
        step of a graph key -- the key holds the record -- runs outside any capture."""
        if record is None or record.alpha is None:
            return None
        t = self._dev.get(record)
        if t is None or t.device != device:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('CriterionState: alpha of a new criterion record must be uploaded outside a capture')
            t = self._dev.put(record, torch.tensor(record.alpha, dtype=torch.float32, device=device))
        return t


def _release(st):
    st['graph'] = st['in'] = st['out'] = None
    ops.clear_rows_cache()      # may hold a tensor of the freed pool


class ReplayedStep:
    """A training step replayed as ONE hipGraph per key.  The subclass supplies `_opts()` (its optimizers), `_graph_key(...)`
    (everything a captured step bakes in by value) and `_eager_step(*batch)` -> one tensor or a tuple of tensors; it counts
    in `_rows_host` what its eager step counts on the host, so that a replay can add the same.  The first step of a key runs
    eagerly under the feeder's recording(), the second is captured, later ones copy the batch into the static inputs, refill
    the starts and replay; a key whose capture failed stays eager, with the reason in `why`.  At most `max_graphs` captured
    steps are kept (least recently used first out)."""

    def __init__(self, max_graphs, rows):
        self.max_graphs = int(max_graphs)
        self._graphs = LRU(self.max_graphs, _release)
        self.stats = {'planned': 0, 'captured': 0, 'replayed': 0, 'refused': 0}
        self.why = None                                     # reason of the last refusal
        self._rows_host = [0] * rows

    def _plan_generations(self):
        return plan_generations(self._opts())

    def _graph_step(self, batch):
        key = self._graph_key(batch)
        for o in self._opts():                              # a schedule step since the last replay: new lr -> device
            if hasattr(o, 'refresh_device_scalars'):
                o.refresh_device_scalars()
        self._graphs.limit = self.max_graphs
        st = self._graphs.get(key)
        if st is not None and st['gens'] is not None and st['gens'] != self._plan_generations():
            del self._graphs[key]                           # raw pointers into a freed Adam plan: never replay
            _release(st)
            st = None
        if st is None:                                      # first step of the key: eager, the feeder records the start plan
            st = self._graphs.put(key, {'feeder': StartFeeder(batch[0].device), 'graph': None, 'in': None, 'out': None,
                                        'gens': None, 'why': None, 'rows': (), 'single': True})
            self.stats['planned'] += 1
            with st['feeder'].recording():
                out = self._eager_step(*batch)
            st['feeder'].build()
            return out
        if st['why'] is not None:                           # a refused key stays eager, in this process
            return self._eager_step(*batch)
        if st['graph'] is None:
            try:
                self._capture(st, batch)
            except Exception as e:
                _release(st)
                st['why'] = self.why = refusal_text(e)
                self.stats['refused'] += 1
                for o in self._opts():                      # gradients of the aborted capture point into its discarded pool
                    o.zero_grad(set_to_none=True)
                return self._eager_step(*batch)
            st['gens'] = self._plan_generations()
            self.stats['captured'] += 1
        for dst, src in zip(st['in'], batch):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        st['feeder'].refill()
        st['graph'].replay()
        self.stats['replayed'] += 1
        for i, n in enumerate(st['rows']):                  # rows the captured step counts on the host
            self._rows_host[i] += n
        out = st['out'].clone()                             # the caller's own: the next replay overwrites the static tensor
        return out if st['single'] else out.unbind(0)

    def _capture(self, st, batch):
        st['in'] = [t.clone() for t in batch]
        for o in self._opts():
            o.zero_grad(set_to_none=True)
        st['graph'] = torch.cuda.CUDAGraph()
        rows0 = list(self._rows_host)
        with st['feeder'].providing(), ops.capture_guard(), torch.cuda.graph(st['graph']):
            outs, st['single'] = tensor_outputs(self._eager_step(*st['in']))
            st['out'] = outs[0] if st['single'] else torch.stack(outs)     # a tuple: one static tensor, one clone per replay
        st['rows'] = tuple(a - b for a, b in zip(self._rows_host, rows0))
        self._rows_host[:] = rows0                          # (a capture runs nothing: its host count is taken back)
        ops.clear_rows_cache()
