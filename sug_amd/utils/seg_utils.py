"""Part-segmentation evaluation with the books on the device: PartIoUMeter (the ShapeNet-Part protocol through
ops.part_iou_accumulate) and seg_eval_worker (model in eval mode over batches of (points, category, label)).

The usual protocol loops over the shapes of every batch on the host in numpy and waits for the device once per batch; here a
batch is two launches and an evaluation reads the device once, at the end.
"""
import numpy as np
import torch

from .. import ops


class PartIoUMeter:
    """part_first / part_count: the categories' contiguous part ranges (host lists or arrays, one entry per category)."""

    def __init__(self, part_first, part_count, device):
        self.part_first, self.part_count = ops.part_table(part_first, part_count)
        self.num_category = int(self.part_first.shape[0])
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('sug_amd ops run on a HIP device only (got %s); there is no CPU fallback' % self.device)
        self.state = ops.part_iou_state(self.device)

    def reset(self):
        self.state.zero_()

    def update(self, logits, label, category):
        """logits [B, N, C] fp32, label [B, N] int64, category [B] int64 on the device.  No host wait."""
        ops.part_iou_accumulate(logits.detach(), label, category, self.part_first, self.part_count, self.state)

    def result(self):
        """One host read -> dict: instance_miou (mean shape IoU over all shapes), class_miou (mean over the categories seen
        of their mean shape IoU), accuracy (points), part_avg_accuracy (mean over the parts seen of their accuracy),
        category_miou [K] (NaN for a category never seen), category_shapes [K], shapes.  Raises if a cloud was not scored."""
        f = ops.part_iou_state_fields(self.state)
        if f['error']:
            raise IndexError('PartIoUMeter: %d cloud(s) with a category outside [0, %d) or a label outside the category\'s part '
                             'range were not scored' % (f['error'], self.num_category))
        K = self.num_category
        iou, shapes = f['cat_iou'][:K], f['cat_shapes'][:K]
        seen = shapes > 0
        with np.errstate(invalid='ignore', divide='ignore'):
            cat_miou = iou / shapes
            part_acc = f['part_correct'] / f['part_points'].astype(np.float64)
        parts_seen = f['part_points'] > 0
        total = int(shapes.sum())
        return {
            'instance_miou': float(iou[seen].sum() / total) if total else float('nan'),
            'class_miou': float(cat_miou[seen].mean()) if seen.any() else float('nan'),
            'accuracy': f['correct'] / f['points'] if f['points'] else float('nan'),
            'part_avg_accuracy': float(part_acc[parts_seen].mean()) if parts_seen.any() else float('nan'),
            'category_miou': cat_miou,
            'category_shapes': shapes.copy(),
            'shapes': f['shapes'],
        }


def seg_eval_worker(model, batches, meter, class_weight=None, ignore_index=-100):
    """Run `model` in eval mode over an iterable of (points [B, 3 + extra, N], category [B], label [B, N]); feed `meter`
    (reset first) and the loss books; ONE host read at the end -> meter.result() plus 'loss' (the mean of the batches'
    cross entropy weighted by their counting rows) and 'rows'.  The model's mode is put back."""
    was_training = model.training
    model.eval()
    meter.reset()
    device = meter.device
    totals = torch.zeros(2, dtype=torch.float64, device=device)
    w = None if class_weight is None else class_weight.detach().to(device=device, dtype=torch.float32)
    try:
        with torch.no_grad():
            for points, category, label in batches:
                points, category, label = points.to(device), category.to(device).long(), label.to(device).long()
                logits, _ = model(points, category)
                ops.point_ce(logits, label, w, ignore_index, totals=totals)
                meter.update(logits, label, category)
    finally:
        model.train(was_training)
    # the one host read: the loss books ride in front of the meter's state block
    block = torch.cat([totals.view(torch.int64), meter.state]).cpu()
    loss_total, rows = block[:2].view(torch.float64).tolist()
    saved = meter.state
    try:
        meter.state = block[2:]
        out = meter.result()
    finally:
        meter.state = saved
    out['loss'] = loss_total / rows if rows else float('nan')
    out['rows'] = rows
    return out
