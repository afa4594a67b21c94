"""One part-segmentation training step, launched eagerly:

  forward -> ops.point_ce (per-point cross entropy, device books) -> backward -> ONE Adam over model.parameters() -> zero_grad.

The public surface of SourceStep: `step`, `set_epoch` (the same cosine schedule) and `epoch_totals` -- the one host read of an
epoch, here (loss total, counting rows, correctly predicted points).  The loss total and the rows are advanced by the loss
kernel's fold, the correct points by one comparison of its arg-max with the labels, summed on the device.  Nothing else in
the step waits for the device.  Graph capture / replay of the step is not offered.
"""
import math

import torch

from . import ops
from .graph_replay import adam_choice


class SegStep:
    def __init__(self, model, lr=1e-3, weight_decay=1e-4, class_weight=None, ignore_index=-100, fused_adam=None):
        self.model = model
        self.base_lr = float(lr)
        self.ignore_index = int(ignore_index)
        p0 = next(model.parameters())
        ops._need_gpu(p0, class_weight)
        self.device = p0.device
        self.class_weight = None if class_weight is None else class_weight.detach().to(device=self.device, dtype=torch.float32)
        self.use_graph = False
        AdamCls, kw = adam_choice(True, fused_adam, False)
        self.optimizer = AdamCls(model.parameters(), lr=lr, weight_decay=weight_decay, **kw)
        # (loss total, counting rows) advanced by sug_point_ce_fwd's fold, then the correctly predicted points: one block,
        # one host read
        self._books = torch.zeros(3, dtype=torch.float64, device=self.device)

    def set_epoch(self, epoch, max_epoch_num):
        """The learning rate at the start of `epoch`: CosineAnnealingLR(T_max=max_epoch_num, eta_min=0) in its closed form, as
        SourceStep.set_epoch sets it.  Returns the rate."""
        lr = self.base_lr * (1 + math.cos(math.pi * epoch / max_epoch_num)) / 2
        for g in self.optimizer.param_groups:
            g['lr'] = lr
        return lr

    def epoch_totals(self, reset=True):
        """(loss total, rows, correct points) since the last reset, as Python floats: the one host read of an epoch.  The loss
        total is the sum over the steps of loss * counting rows, rows the counting rows (labels != ignore_index)."""
        loss_total, rows, correct = self._books.tolist()
        if reset:
            self._books.zero_()
        return float(loss_total), float(rows), float(correct)

    def step(self, points, category, label):
        """points [B, 3 + extra, N] fp32, category [B] int64, label [B, N] int64, all on the HIP device -> the step's loss as a
        0-d device tensor.  No host wait."""
        ops._need_gpu(points, category, label)
        if label.dtype != torch.int64 or label.dim() != 2 or label.shape[0] != points.shape[0] or label.shape[1] != points.shape[-1]:
            raise RuntimeError('SegStep.step: label int64 [B, N] for points [B, C, N] (got %s %s, %s)'
                               % (tuple(label.shape), label.dtype, tuple(points.shape)))
        with ops.deferred_bn_counts():
            logits, _ = self.model(points, category)
        loss, pred = ops.point_ce(logits, label, self.class_weight, self.ignore_index, totals=self._books[:2], want_pred=True)
        with torch.no_grad():
            self._books[2:].add_((pred == label).sum())
        loss.backward()
        ops.clear_rows_cache()
        self.optimizer.step()
        self.optimizer.zero_grad()
        return loss.detach()
