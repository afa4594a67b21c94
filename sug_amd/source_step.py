"""One source-only training step (BASELINE configuration 1), mirroring the batch loop of the reference's
train_source.py:104-136 and its optimiser set-up (:86, :95-96):

  forward -> criterion (+ p2p_fitting_regularizer for KPFCls, :122-124) -> backward -> ONE Adam over model.parameters() ->
  zero_grad, with `loss_total += loss_s.item() * data.size(0); data_total += data.size(0)` (:130-131) kept on the device.

For Pointnet_cls, Pointnet2_cls, model_pointnet.DGCNN and PointTransformerCls the step follows the plan / capture / replay
protocol of graph_replay.py as SUGStep's graph step does: the first step of a key runs eagerly under the FPS start feeder's
recording(), the second is captured, later ones copy the batch into the static inputs, refill the starts and replay.  A plain
nn.CrossEntropyLoss (no weight, reduction 'mean', C <= 64) runs as ops.ce, whose one launch also advances the epoch totals; any
other criterion is called as it is and its loss is added to the totals by one in-place add.  Nothing waits for the device
until `epoch_totals()` -- the one host read of an epoch.

`use_graph=False` launches the same ops eagerly: the graph's bit-for-bit twin (tests/test_gpu_source_step.py).
"""
import contextlib
import math

import torch
import torch.nn as nn

from . import ops
from .graph_replay import LRU, StartFeeder, refusal_text


def _release(st):
    st['graph'] = st['in'] = st['out'] = None
    ops.clear_rows_cache()      # may hold a tensor of the freed pool


class SourceStep:
    def __init__(self, model, lr=1e-3, weight_decay=5e-5, criterion=None, use_graph=True, fused_adam=None, max_graphs=4):
        self.model = model
        self.base_lr = float(lr)
        self.criterion = criterion if criterion is not None else nn.CrossEntropyLoss()
        p0 = next(model.parameters())
        self.device = p0.device
        on_gpu = p0.is_cuda
        # fused_adam: None/True -> sug_amd.optim.Adam (one launch) on a HIP device; False -> torch.optim.Adam
        own_adam = on_gpu and (fused_adam is None or fused_adam)
        self.use_graph = bool(use_graph) and on_gpu
        # a model whose level sizes depend on the data (KPFCls) has no static launch sequence: always eager
        self.why = None                                 # reason of the last refusal
        if self.use_graph and not (getattr(model, 'graph_capturable', True) and
                                   getattr(getattr(model, 'g', None), 'graph_capturable', True)):
            self.use_graph = False
            self.why = '%s: level sizes depend on the data' % type(model).__name__
        kw = {}
        if own_adam:
            from .optim import Adam as AdamCls
            kw['graph_capturable'] = True               # step count / bias corrections / lr on the device, in both launch modes
        else:
            AdamCls = torch.optim.Adam
            if self.use_graph:
                kw['capturable'] = True
                kw['fused'] = True
        self.optimizer = AdamCls(model.parameters(), lr=lr, weight_decay=weight_decay, **kw)      # train_source.py:95
        self.max_graphs = int(max_graphs)
        self._graphs = LRU(self.max_graphs, _release)
        self.stats = {'planned': 0, 'captured': 0, 'replayed': 0, 'refused': 0}
        # (loss_total, data_total) of train_source.py:110-111, :130-131; rows of steps whose criterion is not the fused
        # kernel are counted on the host (their number is known there)
        self._totals = torch.zeros(2, dtype=torch.float64, device=self.device) if on_gpu else None
        self._rows_host = 0
        from .model.KPConv_model import KPFCls
        self._kpf = isinstance(model, KPFCls)

    # ------------------------------------------------------------------ learning-rate schedule
    def set_epoch(self, epoch, max_epoch_num):
        """The learning rate at the start of `epoch` as the reference sets it (train_source.py:96, :106):
        CosineAnnealingLR(T_max=max_epoch_num, eta_min=0) stepped with an explicit epoch, i.e. its closed form.  With
        sug_amd.optim.Adam the rate lives on the device: one captured graph serves every epoch.  Returns the rate."""
        lr = self.base_lr * (1 + math.cos(math.pi * epoch / max_epoch_num)) / 2
        for g in self.optimizer.param_groups:
            g['lr'] = lr
        return lr

    # ------------------------------------------------------------------ the epoch's books
    def epoch_totals(self, reset=True):
        """(loss_total, data_total) since the last reset, as Python floats: the one host read of an epoch (what
        train_source.py:134 prints every ten batches as loss_total / data_total)."""
        if self._totals is None:
            return 0.0, 0.0
        loss_total, rows = self._totals.tolist()
        rows += self._rows_host
        if reset:
            self._totals.zero_()
            self._rows_host = 0
        return float(loss_total), float(rows)

    # ------------------------------------------------------------------ step
    def step(self, data, label):
        """data [B,3,N,1] fp32, label [B] int64, both on the HIP device -> the step's loss as a 0-d device tensor of the
        caller's own (a replay does not overwrite it).  No host wait."""
        ops._need_gpu(data, label, next(self.model.parameters()))
        if data.dim() != 4 or data.shape[0] != label.shape[0] or label.dtype != torch.int64:
            raise RuntimeError('SourceStep.step: data [B,3,N,1] and label int64 [B] (got %s, %s %s)' %
                               (tuple(data.shape), tuple(label.shape), label.dtype))
        if self.use_graph:
            return self._graph_step(data, label)
        return self._eager_step(data, label)

    def _plain_ce(self):
        c = self.criterion
        return type(c) is nn.CrossEntropyLoss and c.weight is None and c.reduction == 'mean'

    def _graph_key(self, data, label):
        """Everything a captured step bakes in by value.  sug_amd.optim.Adam keeps lr on the device; torch's takes it by
        value, so there it is part of the key."""
        from .model import Ptran_transformer as PT
        c, o = self.criterion, self.optimizer
        crit = ('ce', int(c.ignore_index), float(c.label_smoothing)) if self._plain_ce() else ('call', id(c), repr(c))
        hyp = o.graph_key() if hasattr(o, 'graph_key') else \
            tuple((g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) for g in o.param_groups)
        return (tuple(data.shape), tuple(label.shape), crit, self.model.training, PT.GEMM_DTYPE,
                getattr(PT, 'PROJ_16BIT', None), hyp)

    def _graph_step(self, data, label):
        key = self._graph_key(data, label)
        opt = self.optimizer
        if hasattr(opt, 'refresh_device_scalars'):          # a schedule step since the last replay: new lr -> device
            opt.refresh_device_scalars()
        self._graphs.limit = self.max_graphs
        st = self._graphs.get(key)
        if st is not None and st['gens'] is not None and st['gens'] != getattr(opt, 'plan_generation', 0):
            del self._graphs[key]                           # raw pointers into a freed Adam plan: never replay
            _release(st)
            st = None
        if st is None:                                      # first step of the key: eager, the feeder records the start plan
            st = self._graphs.put(key, {'feeder': StartFeeder(data.device), 'graph': None, 'in': None, 'out': None,
                                        'gens': None, 'why': None, 'fused_books': True})
            self.stats['planned'] += 1
            with st['feeder'].recording():
                out = self._eager_step(data, label)
            st['feeder'].build()
            return out
        if st['why'] is not None:                           # a refused key stays eager, in this process
            return self._eager_step(data, label)
        if st['graph'] is None:
            try:
                self._capture(st, data, label)
            except Exception as e:
                _release(st)
                st['why'] = self.why = refusal_text(e)
                self.stats['refused'] += 1
                opt.zero_grad(set_to_none=True)             # gradients of the aborted capture point into its discarded pool
                return self._eager_step(data, label)
            st['gens'] = getattr(opt, 'plan_generation', 0)
            self.stats['captured'] += 1
        for dst, src in zip(st['in'], (data, label)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        st['feeder'].refill()
        st['graph'].replay()
        self.stats['replayed'] += 1
        if not st['fused_books']:
            self._rows_host += data.shape[0]
        return st['out'].clone()                            # the caller's own tensor: the next replay overwrites the static one

    def _capture(self, st, data, label):
        st['in'] = [data.clone(), label.clone()]
        self.optimizer.zero_grad(set_to_none=True)
        st['graph'] = torch.cuda.CUDAGraph()
        rows0 = self._rows_host
        with st['feeder'].providing(), ops.capture_guard(), torch.cuda.graph(st['graph']):
            st['out'] = self._eager_step(*st['in'])
        st['fused_books'] = self._rows_host == rows0        # (a capture runs nothing: its host count is taken back)
        self._rows_host = rows0
        ops.clear_rows_cache()

    @contextlib.contextmanager
    def _step_scope(self):
        """The forward of one step: 16-bit weight copies (Point Transformer, fp16 mode) shared by its calls -- from the second
        step on refreshed by one multi-tensor copy into the first step's buffers -- and every num_batches_tracked increment
        in one launch."""
        from .model import Ptran_transformer as _PT
        ops.CTX.w16_cache = ops.w16_prefill(getattr(self, '_w16_plan', None) or []) if _PT.GEMM_DTYPE is not None else None
        try:
            with ops.deferred_bn_counts():
                yield
        finally:
            if ops.CTX.w16_cache is not None:
                self._w16_plan = ops.w16_plan(ops.CTX.w16_cache)
            ops.CTX.w16_cache = None

    def _eager_step(self, data, label):
        model, B = self.model, data.shape[0]
        with self._step_scope():
            out = model(data)
        reg = 0
        if self._kpf:                                       # train_source.py:122-124
            from .model.KPConv_model import p2p_fitting_regularizer
            reg = p2p_fitting_regularizer(model.encoder.encoder_blocks, deform_fitting_power=model.deform_fitting_power)
        no_reg = isinstance(reg, (int, float)) and reg == 0
        if self._plain_ce() and no_reg and out.dim() == 2 and ops.ce_supported(out, label):
            c = self.criterion
            loss = ops.ce(out, label, c.ignore_index, c.label_smoothing, totals=self._totals)
        else:
            loss = self.criterion(out, label)
            if not no_reg:
                loss = loss + reg
            with torch.no_grad():                           # loss_total += loss * B, in fp64, one launch
                self._totals[0:1].add_(loss.detach().reshape(1), alpha=B)
            self._rows_host += B
        loss.backward()
        ops.clear_rows_cache()
        self.optimizer.step()
        self.optimizer.zero_grad()
        return loss.detach()
