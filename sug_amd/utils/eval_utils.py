"""Drop-in eval_worker (utils/eval_utils.py:5-88 of the reference): `from sug_amd.utils.eval_utils import eval_worker`.

Same eval_dict keys, same result dict (`pred_acc` a 0-dim float64 device tensor, as `correct_total.double() / data_total`
is there), same quantities logged.  What changes is where the work runs:

  * the forward goes through eval_graphs (hipGraph replay of the eval-mode call on a private model copy, refreshed from the
    model handed in), or the eager call where eval_graphs declines;
  * each batch's metrics are ONE launch of sug_eval_accumulate (ops.eval_accumulate): averaged heads, argmax, the
    cross entropy when the criterion is a plain nn.CrossEntropyLoss (any other criterion -- focal_loss -- is called as is,
    once per batch, on the averaged logits, and its device scalar handed to the kernel), integer counts and the fp64
    accumulators, on the device.  The loop does not wait for the device; one synchronisation at the end copies the state
    block to the host, where the per-class and per-batch ratios are assembled exactly as numpy assembles the reference's.

Labels that are not 1-D int64, more than 64 classes or 4096 rows per batch, or a data loader without a length: the loop is
the eager restatement of the same arithmetic (same results, a host synchronisation per batch).  A label outside
[0, num_class) raises IndexError (at the end of the call on the device path).
"""
import weakref

import numpy as np
import torch
import torch.nn as nn

from .. import eval_graphs, ops

# what the last eval_worker call did: 'form' ('device' | 'eager'), 'syncs' (host waits for the device), 'graphs'
# (forward through eval_graphs), 'why' (the reason of an eager form), and the logged quantities
LAST = {}


def _fused_ce(criterion):
    """(reduction, ignore_index, label_smoothing) when `criterion` is a plain nn.CrossEntropyLoss the kernel can compute."""
    if type(criterion) is nn.CrossEntropyLoss and criterion.weight is None and criterion.reduction in ('mean', 'sum'):
        return (criterion.reduction, int(criterion.ignore_index), float(criterion.label_smoothing))
    return None


def assemble(class_acc2, batch_acc, num_class):
    """End-of-loop arithmetic from the accumulators: class_acc [num_class, 3] with column 2 = column 0 / column 1 (0/0 ->
    NaN for classes never seen), its mean, and instance_acc = np.mean of the per-batch ratios."""
    class_acc = np.zeros((num_class, 3))
    class_acc[:, :2] = class_acc2[:num_class]
    with np.errstate(invalid='ignore', divide='ignore'):
        class_acc[:, 2] = class_acc[:, 0] / class_acc[:, 1]
    class_acc_mean = np.mean(class_acc[:, 2])
    instance_acc = np.mean(list(batch_acc))
    return class_acc, class_acc_mean, instance_acc


class _Eager:
    """The per-batch arithmetic on the host (one synchronisation per batch and more); continues a device state block."""

    def __init__(self, num_class, fields=None):
        self.class_acc = np.zeros((num_class, 2))
        self.batch_acc, self.loss_total, self.correct_total, self.data_total = [], 0.0, 0, 0
        if fields is not None:
            self.class_acc[:] = fields['class_acc'][:num_class]
            self.batch_acc = [float(v) for v in fields['batch_acc']]
            self.loss_total, self.correct_total, self.data_total = fields['loss_total'], fields['correct_total'], fields['data_total']

    def add(self, output, label, criterion, per_class):
        lab = label.cpu().numpy()
        if lab.size and (lab.min() < 0 or lab.max() >= self.class_acc.shape[0]):
            raise IndexError('eval_worker: label outside [0, %d)' % self.class_acc.shape[0])
        loss = criterion(output, label)
        pred = torch.max(output, 1)[1].cpu().numpy()
        B = int(output.shape[0])
        if per_class:
            for j in np.unique(lab):
                sel = lab == j
                self.class_acc[j, 0] += int((pred[sel] == j).sum()) / float(int(sel.sum()))
                self.class_acc[j, 1] += 1
        correct = int((pred == lab).sum())
        self.batch_acc.append(correct / float(B))
        self.loss_total += loss.item() * B
        self.correct_total += correct
        self.data_total += B


def eval_worker(eval_dict, logger):
    model = eval_dict['model']
    dataloader = eval_dict['dataloader']
    best_target_acc = eval_dict['best_target_acc']
    dataset = eval_dict['dataset']
    device = eval_dict['device']
    criterion = eval_dict['criterion']
    epoch = eval_dict['epoch']
    best_target_acc_epoch = eval_dict['best_target_acc_epoch']
    num_class = eval_dict['num_class']
    source_flag = 'source_flag' in eval_dict
    cls_eval = eval_dict.get('cls_eval', False)
    per_class = source_flag or cls_eval
    logger.info('evaluating %s (%s)' % (dataset, eval_dict.get('dataset_name')))

    fused = _fused_ce(criterion)
    try:
        cap = len(dataloader)
    except TypeError:
        cap = None
    why = None if cap else 'data loader without a length'
    if why is None and not 1 <= num_class <= ops.EVAL_MAX_CLASSES:
        why = 'num_class %d' % num_class
    why_graphs = eval_graphs.fallback_reason(model, torch.empty(0, device=device))
    if why_graphs is not None and why_graphs != 'input':
        eval_graphs.FALLBACKS[why_graphs] += 1
    runner = None
    if why_graphs is None:
        runner = eval_graphs.runner_for(model)
        runner.refresh(model)

    state, eager, syncs = None, None, 0
    for data, label in dataloader:
        data = data.to(device=device)
        label = label.to(device=device).long()
        out = None
        if runner is not None:
            out = runner.run(data, clone=False)
            if out is None:
                eval_graphs.FALLBACKS['capture refused'] += 1
        if out is None:
            out = model(data)
        l1, l2 = (out, None) if source_flag else (out[0], out[1])
        ok = why is None and eager is None and ops.eval_accumulate_supported(l1, label) and l1.shape[1] == num_class
        if ok and l2 is not None:
            ok = l2.shape == l1.shape and l2.stride() == l1.stride()
        with torch.no_grad():
            if ok:
                if state is None:
                    state = ops.eval_state(cap, data.device)
                if fused is not None:
                    ops.eval_accumulate(state, l1, label, logits2=l2, ce=fused, cls_eval=per_class)
                else:
                    output = l1 if l2 is None else (l1 + l2) / 2
                    ops.eval_accumulate(state, output, label, loss=criterion(output, label), cls_eval=per_class)
                continue
            if eager is None:
                why = why or 'batch of shape %s, labels %s %s' % (tuple(l1.shape), label.dtype, tuple(label.shape))
                fields = None
                if state is not None:           # continue the device accumulators on the host, in the same order
                    fields = ops.eval_state_fields(state)
                    syncs += 1
                    _raise_on_error(fields, num_class)
                eager = _Eager(num_class, fields)
            output = l1 if l2 is None else (l1 + l2) / 2
            eager.add(output, label, criterion, per_class)
            syncs += 3                          # label.cpu(), pred.cpu(), loss.item()

    if eager is None and state is not None:
        f = ops.eval_state_fields(state)        # the one synchronisation of the device form
        syncs += 1
        _raise_on_error(f, num_class)
        class_acc2, batch_acc = f['class_acc'], f['batch_acc']
        loss_total, correct_total, data_total = f['loss_total'], f['correct_total'], f['data_total']
        correct_dev = state[ops.EVAL_CORRECT_TOTAL]
    elif eager is not None:
        class_acc2, batch_acc = eager.class_acc, eager.batch_acc
        loss_total, correct_total, data_total = eager.loss_total, eager.correct_total, eager.data_total
        correct_dev = torch.tensor(correct_total, dtype=torch.int64, device=device)
    else:
        raise ZeroDivisionError('eval_worker: empty data loader')

    pred_loss = loss_total / data_total
    pred_acc = correct_dev.double() / data_total          # 0-dim float64 on the device, as the reference's
    acc_host = correct_total / float(data_total)           # the same IEEE division: no second synchronisation to compare
    class_acc, class_acc_mean, instance_acc = assemble(class_acc2, batch_acc, num_class)

    _remember(pred_acc, acc_host)
    best_host = _host_value(best_target_acc)
    if acc_host > best_host:
        best_target_acc, best_host = pred_acc, acc_host
        best_target_acc_epoch = epoch
    logger.info('%s epoch %s: accuracy %r, best %r (epoch %s), loss %r'
                % (dataset, epoch, acc_host, best_host, best_target_acc_epoch, pred_loss))
    if per_class:
        logger.info('%s per-class accuracy: %s' % (dataset, np.array2string(class_acc[:, 2], precision=6)))
        logger.info('%s instance accuracy %r, mean class accuracy %r' % (dataset, instance_acc, class_acc_mean))

    LAST.clear()
    LAST.update(form='eager' if eager is not None else 'device', why=why, graphs=runner is not None, syncs=syncs,
                batches=len(batch_acc), class_acc=class_acc, class_acc_mean=class_acc_mean, instance_acc=instance_acc,
                pred_loss=pred_loss, correct_total=correct_total, data_total=data_total,
                stats=dict(runner.stats) if runner is not None else None)
    return {
        'dataset': dataset,
        'epoch': epoch,
        'best_target_acc': best_target_acc,
        'best_target_acc_epoch': best_target_acc_epoch,
        'cur_target_acc': pred_acc,
    }


# host values of the accuracies this module returned (the next call compares against its best without reading the device)
_HOST = {}                  # id(tensor) -> (weak reference, value)


def _remember(t, v):
    for k in [k for k, (r, _) in _HOST.items() if r() is None]:
        del _HOST[k]
    _HOST[id(t)] = (weakref.ref(t), v)


def _host_value(v):
    if isinstance(v, torch.Tensor):
        hit = _HOST.get(id(v))
        if hit is not None and hit[0]() is v:
            return hit[1]
    return float(v)


def _raise_on_error(fields, num_class):
    if fields['error'] & 1:
        raise IndexError('eval_worker: a label outside [0, %d)' % num_class)
    if fields['error'] & 2:
        raise RuntimeError('eval_worker: more batches than len(dataloader) = %d' % (len(fields['batch_acc'])))
