"""hipGraph replay of the EVAL-mode forward -- what eval_worker (utils/eval_utils.py) calls once per test batch.

The reference evaluates every epoch on three test sets with `model(data)` in eval mode under torch.no_grad() on a fresh
`copy.deepcopy(model)` (train_dg_single_gpu.py:360-383).  Per-call graphs (call_graphs.py) serve train-mode calls only, so
that loop launches kernel by kernel from Python.  This module replays it instead:

  * a runner owns ONE private copy of the model per architecture signature (module class, backbone, state_dict names /
    shapes / dtypes, device, Point Transformer GEMM dtype): graphs captured against the caller's fresh deepcopy would be
    captured again every epoch.  At the start of an evaluation (refresh) the copy's parameters and buffers are overwritten
    from the model handed in, with one multi-tensor copy per dtype.  Everything the copy inherited that could hold tensors
    made outside the graph is cleared (the EdgeConv weight-split cache, the encoder prefix cache, a call-graph manager) and
    the 16-bit weight cache is off inside the runner, so the derived weights -- the [W1; W2-W1] split, fp16 casts, the
    BatchNorm eval coefficients -- are recomputed inside the graph on every replay from the refreshed storage;
  * a key is (signature, input shape, forward flags).  Its first call runs eagerly on the copy and records the
    farthest-point-sampling start plan; the second is captured (torch.no_grad, ops.capture_guard) and replayed at once; later
    calls copy the batch into the static input, draw the FPS starts from the CPU generator in call order
    (graph_replay.StartFeeder: the random stream of the eager calls) and replay.  The last, partial batch of a test set is
    a key of its own and replays from the second epoch on;
  * at most MAX_KEYS keys per runner and MAX_RUNNERS runners, least recently used first out (their graph pools are freed);
  * the eager call on the model handed in is used instead -- and the reason recorded in FALLBACKS -- when the model is in
    train mode, a scoped ops.CTX field is set, a capture is in progress, the module is not one this runner knows, or the
    capture of the key raised (`why` of the runner).

`EvalRunner(model)(x, **flags)` refreshes from `model` and returns clones of the outputs; eval_worker uses run() without
clones -- its metrics kernel consumes the static outputs in stream order before the next replay.
"""
import collections
import copy
import inspect
import weakref

import torch

from . import ops
from .graph_replay import LRU, StartFeeder, refusal_text, tensor_outputs

MAX_KEYS = 8
MAX_RUNNERS = 2

FALLBACKS = collections.Counter()           # reason -> eager calls on the caller's model


def _known_types():
    from .model.Model import Net_MDA
    from .model.model_pointnet import Pointnet_cls, Pointnet2_cls, DGCNN
    from .model.Ptran_model import PointTransformerCls
    return (Net_MDA, Pointnet_cls, Pointnet2_cls, DGCNN, PointTransformerCls)


def signature(model):
    """Architecture signature: models with equal signatures can share one private copy."""
    from .model import Ptran_transformer as PT
    sd = model.state_dict(keep_vars=True)
    dev = str(next(iter(sd.values())).device) if sd else None
    g = getattr(model, 'g', None)
    caps = getattr(g, 'level_caps', None)                   # KPConv_g: the capacities size the private copy's launches
    return (type(model).__module__ + '.' + type(model).__qualname__,
            None if g is None else type(g).__qualname__ + ('' if caps is None else ' caps=%r' % (caps,)),
            tuple((k, tuple(v.shape), str(v.dtype)) for k, v in sd.items()), dev, str(PT.GEMM_DTYPE),
            str(getattr(PT, 'PROJ_16BIT', None)))


def fallback_reason(model, x):
    """Why a call cannot go through a runner (None: it can)."""
    if not isinstance(model, _known_types()):
        return 'module %s' % type(model).__name__
    if not getattr(getattr(model, 'g', None), 'graph_capturable', True):
        return 'KPConv: level sizes depend on the data (set_level_caps fixes them)'
    if any(m.training for m in model.modules()):
        return 'train mode'
    if not ops.CTX.unscoped():
        return 'scoped ops.CTX field'
    if torch.cuda.is_current_stream_capturing():
        return 'capture in progress'
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        return 'input'
    return None


class _Key:
    __slots__ = ('graph', 'x', 'feeder', 'outs', 'single', 'eager_only', 'why')

    def __init__(self):
        self.why = None
        self.single = self.eager_only = False
        self.release()

    def release(self):
        self.graph = self.x = self.feeder = self.outs = None


def _release_key(ks):
    ks.release()
    ops.clear_rows_cache()      # may hold a tensor of the freed pool


class EvalRunner:
    """Graph replay of eval-mode forwards of one architecture (see the module docstring)."""

    def __init__(self, model):
        if not isinstance(model, _known_types()):
            raise TypeError('EvalRunner: %s is not Net_MDA / Pointnet_cls / Pointnet2_cls / DGCNN / PointTransformerCls'
                            % type(model).__name__)
        self.sig = signature(model)
        self.net = self._private_copy(model)
        sd = self.net.state_dict(keep_vars=True)
        self._names = list(sd.keys())
        self._dst = [t.detach() for t in sd.values()]
        self.keys = LRU(MAX_KEYS, _release_key)
        self.stats = {'eager': 0, 'captured': 0, 'replayed': 0, 'refused': 0, 'evicted': 0}
        self.why = None                         # reason of the last refused capture
        # Net_MDA's flags in the order of _forward_impl, defaults filled in: equal calls get equal keys
        from .model.Model import Net_MDA
        self._flag_names = list(inspect.signature(Net_MDA._forward_impl).parameters.items())[2:] \
            if isinstance(model, Net_MDA) else None
        self._src = weakref.ref(model)

    def __call__(self, x, **flags):
        """model(x, **flags) in eval mode for the model the runner was made for: refresh from it, run, return clones."""
        model = self._src()
        if model is None:
            raise RuntimeError('EvalRunner: the model it was made for is gone')
        return forward(model, x, flags, clone=True, runner=self)

    # ------------------------------------------------------------------ private copy
    @staticmethod
    def _private_copy(model):
        keep = model.__dict__.pop('_call_graph_mgr', None)
        try:
            net = copy.deepcopy(model)
        finally:
            if keep is not None:
                model.__dict__['_call_graph_mgr'] = keep
        net.__dict__.pop('_call_graph_mgr', None)
        for m in net.modules():
            if hasattr(m, 'cache_weight_split'):
                m.cache_weight_split = False
                m._wcat = None
            if hasattr(m, '_prefix_cache'):
                m._prefix_cache = {}
            if '_geometry' in m.__dict__:
                m._geometry = None
        for p in net.parameters():
            p.grad = None
        return net.eval()

    def refresh(self, model):
        """Overwrite the private copy's parameters and buffers with `model`'s (one multi-tensor copy per dtype)."""
        sd = model.state_dict(keep_vars=True)
        if list(sd.keys()) != self._names:
            raise RuntimeError('EvalRunner.refresh: state_dict names differ from the runner signature')
        groups = {}
        for d, s in zip(self._dst, sd.values()):
            dd, ss = groups.setdefault(d.dtype, ([], []))
            dd.append(d)
            ss.append(s.detach())
        with torch.no_grad():
            for dd, ss in groups.values():
                torch._foreach_copy_(dd, ss)

    # ------------------------------------------------------------------ keys
    def _flags(self, flags):
        if self._flag_names is not None:
            return tuple((n, flags.get(n, prm.default)) for n, prm in self._flag_names)
        return tuple(sorted(flags.items()))

    def key_state(self, key):
        ks = self.keys.get(key)
        if ks is None:
            before = len(self.keys)
            ks = self.keys.put(key, _Key())
            if len(self.keys) == before:
                self.stats['evicted'] += 1
        return ks

    def release(self):
        for ks in self.keys.values():
            _release_key(ks)
        self.keys.clear()

    # ------------------------------------------------------------------ the call
    def run(self, x, flags=None, clone=True):
        """The private copy's eval-mode forward on x (refresh() first): eager, captured or replayed."""
        flags = dict(flags or {})
        nflags = self._flags(flags)
        ks = self.key_state((self.sig, tuple(x.shape), nflags))
        with torch.no_grad():
            if ks.eager_only:
                self.stats['eager'] += 1
                return self._plain(x, flags)
            if ks.feeder is None:               # first call of the key: eager, the feeder records the start plan
                return self._eager_plan(ks, x, flags)
            if ks.graph is None:
                try:
                    self._capture(ks, x, flags)
                except Exception as e:       # this key stays eager, in this process
                    ks.release()
                    ks.eager_only = True
                    ks.why = self.why = refusal_text(e)
                    self.stats['refused'] += 1
                    return None
                self.stats['captured'] += 1
            ks.x.copy_(x, non_blocking=True)
            ks.feeder.refill()
            ks.graph.replay()
            self.stats['replayed'] += 1
            outs = ks.outs
            if clone:
                outs = [o.clone() for o in outs]
            return outs[0] if ks.single else tuple(outs)

    def _plain(self, x, flags):
        with ops.CTX.scoped(w16_cache=None):
            return self.net(x, **flags)

    def _eager_plan(self, ks, x, flags):
        self.stats['eager'] += 1
        feeder = StartFeeder(x.device)
        with feeder.recording():
            out = self._plain(x, flags)
        ks.feeder = feeder              # (unbuilt: _capture gives it its buffers)
        return out

    def _capture(self, ks, x, flags):
        ks.x = x.detach().clone()
        ks.feeder.build()
        ks.graph = torch.cuda.CUDAGraph()
        with ops.CTX.scoped(w16_cache=None), ks.feeder.providing(), ops.capture_guard(), \
                torch.cuda.graph(ks.graph, capture_error_mode='thread_local'):
            out = self.net(ks.x, **flags)
        outs, ks.single = tensor_outputs(out)
        if not outs or not all(isinstance(t, torch.Tensor) for t in outs):
            raise RuntimeError('this forward mode does not return tensors only')
        ks.outs = outs
        # prefix-cache entries or a rows-cache entry made during the capture point into the graph's pool: drop them
        for m in self.net.modules():
            if hasattr(m, '_prefix_cache'):
                m._prefix_cache = {}
        ops.clear_rows_cache()


# ---------------------------------------------------------------------- runners of the process
_RUNNERS = LRU(MAX_RUNNERS, lambda r: r.release())


def runner_for(model):
    """The process's runner for `model`'s signature (made on first use; at most MAX_RUNNERS are kept)."""
    sig = signature(model)
    r = _RUNNERS.get(sig)
    if r is None:
        r = _RUNNERS.put(sig, EvalRunner(model))
    return r


def drop_all():
    """Forget every runner (their private copies and graph pools are released)."""
    for r in _RUNNERS.values():
        r.release()
    _RUNNERS.clear()


def forward(model, x, flags=None, clone=True, runner=None, refresh=True):
    """model(x, **flags) in eval mode: through a runner where possible, the eager call on `model` otherwise."""
    flags = dict(flags or {})
    why = fallback_reason(model, x)
    if why is None:
        r = runner if runner is not None else runner_for(model)
        if refresh:
            r.refresh(model)
        out = r.run(x, flags, clone=clone)
        if out is not None:
            return out
        why = 'capture refused'
    FALLBACKS[why] += 1
    with torch.no_grad():
        return model(x, **flags)
