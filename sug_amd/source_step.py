"""One source-only training step (BASELINE configuration 1), mirroring the batch loop of the reference's
train_source.py:104-136 and its optimiser set-up (:86, :95-96):

  forward -> criterion (+ p2p_fitting_regularizer for KPFCls, :122-124) -> backward -> ONE Adam over model.parameters() ->
  zero_grad, with `loss_total += loss_s.item() * data.size(0); data_total += data.size(0)` (:130-131) kept on the device.

For Pointnet_cls, Pointnet2_cls, model_pointnet.DGCNN and PointTransformerCls the step is a graph_replay.ReplayedStep: planned,
captured and replayed by that class's protocol, one graph per key.  A plain nn.CrossEntropyLoss (no weight, reduction 'mean',
C <= 64) runs as ops.ce, whose one launch also advances the epoch totals; any other criterion is called as it is and its loss
is added to the totals by one in-place add.  Nothing waits for the device until `epoch_totals()` -- the one host read of an
epoch.

`use_graph=False` launches the same ops eagerly: the graph's bit-for-bit twin (tests/test_gpu_source_step.py).
"""
import math

import torch
import torch.nn as nn

from . import ops
from .graph_replay import ReplayedStep, adam_choice, hyper_key, plain_ce


class SourceStep(ReplayedStep):
    def __init__(self, model, lr=1e-3, weight_decay=5e-5, criterion=None, use_graph=True, fused_adam=None, max_graphs=4):
        self.model = model
        self.base_lr = float(lr)
        self.criterion = criterion if criterion is not None else nn.CrossEntropyLoss()
        p0 = next(model.parameters())
        self.device = p0.device
        on_gpu = p0.is_cuda
        super().__init__(max_graphs, rows=1)
        self.use_graph = bool(use_graph) and on_gpu
        # a model whose level sizes depend on the data (KPFCls) has no static launch sequence: always eager
        if self.use_graph and not (getattr(model, 'graph_capturable', True) and
                                   getattr(getattr(model, 'g', None), 'graph_capturable', True)):
            self.use_graph = False
            self.why = '%s: level sizes depend on the data (set_level_caps fixes them)' % type(model).__name__
        AdamCls, kw = adam_choice(on_gpu, fused_adam, self.use_graph)
        self.optimizer = AdamCls(model.parameters(), lr=lr, weight_decay=weight_decay, **kw)      # train_source.py:95
        # (loss_total, data_total) of train_source.py:110-111, :130-131; rows of steps whose criterion is not the fused
        # kernel are counted on the host (their number is known there)
        self._totals = torch.zeros(2, dtype=torch.float64, device=self.device) if on_gpu else None
        from .model.KPConv_model import KPFCls
        self._kpf = isinstance(model, KPFCls)
        self._w16_plan = [None]

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
        from .train_step import check_level_caps
        for m in (self.model, getattr(self.model, 'g', None)):      # KPFCls / a KPConv encoder with level caps: overflow raises
            check_level_caps(m, reset)
        loss_total, rows = self._totals.tolist()
        rows += self._rows_host[0]
        if reset:
            self._totals.zero_()
            self._rows_host[0] = 0
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
            return self._graph_step((data, label))
        return self._eager_step(data, label)

    def _opts(self):
        return (self.optimizer,)

    def _graph_key(self, batch):
        """Everything a captured step bakes in by value."""
        from .model import Ptran_transformer as PT
        c = self.criterion
        crit = ('ce', int(c.ignore_index), float(c.label_smoothing)) if plain_ce(c, smoothing_ok=True) else ('call', id(c), repr(c))
        key = (tuple(batch[0].shape), tuple(batch[1].shape), crit, self.model.training, PT.GEMM_DTYPE,
               getattr(PT, 'PROJ_16BIT', None), hyper_key(self.optimizer))
        caps = getattr(self.model, 'level_caps', None)      # KPFCls: the level capacities size every launch
        return key if caps is None else key + (('level_caps', caps),)

    def _eager_step(self, data, label):
        model, B = self.model, data.shape[0]
        # 16-bit weight copies (Point Transformer, fp16 mode) shared by the forward's calls -- from the second step on refreshed
        # by one multi-tensor copy into the first step's buffers -- and every num_batches_tracked increment in one launch
        with ops.w16_scope(self._w16_plan, 0), ops.deferred_bn_counts():
            out = model(data)
        reg = 0
        if self._kpf:                                       # train_source.py:122-124
            from .model.KPConv_model import p2p_fitting_regularizer
            reg = p2p_fitting_regularizer(model.encoder.encoder_blocks, deform_fitting_power=model.deform_fitting_power)
        no_reg = isinstance(reg, (int, float)) and reg == 0
        if plain_ce(self.criterion, smoothing_ok=True) and no_reg and out.dim() == 2 and ops.ce_supported(out, label):
            c = self.criterion
            loss = ops.ce(out, label, c.ignore_index, c.label_smoothing, totals=self._totals)
        else:
            loss = self.criterion(out, label)
            if not no_reg:
                loss = loss + reg
            with torch.no_grad():                           # loss_total += loss * B, in fp64, one launch
                self._totals[0:1].add_(loss.detach().reshape(1), alpha=B)
            self._rows_host[0] += B
        loss.backward()
        ops.clear_rows_cache()
        self.optimizer.step()
        self.optimizer.zero_grad()
        return loss.detach()
