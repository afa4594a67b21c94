"""The GPU cases of tests/test_gpu_eval_worker.py: sug_eval_accumulate and the drop-in eval_worker (sug_amd.utils.eval_utils)
against a restatement of the reference's evaluation loop (utils/eval_utils.py:37-82) over the eager eval-mode forward --
metrics bit for bit, loss within 1e-6, the CPU generator's stream unchanged, graphs replayed from the second epoch on, and
refreshed weights seen by the replays.

Run as a script in a child process of its own (`python tests/eval_worker_cases.py RESULTS.json`): the runners of
sug_amd.eval_graphs keep private model copies and graph pools alive by design, and a test process that went through them
would hand the tests after this file a different caching-allocator history.  Writes {case id: null | traceback}."""
import copy
import json
import logging
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import ref_cpu as O  # noqa: E402

LOG = logging.getLogger('eval_worker_cases')

KINDS = ('DGCNN', 'Pointnet', 'Pointnet2', 'PTran', 'Pointnet_cls')


# ------------------------------------------------------------------ the reference loop, restated
def restated_loop(model, batches, criterion, num_class, source_flag, cls_eval, best=0.0, best_epoch=0, epoch=0):
    per_class = source_flag or cls_eval
    acc = np.zeros((num_class, 3))
    ratios, loss_sum, n_rows = [], 0, 0
    hits = 0
    for data, label in batches:
        y = model(data)
        output = y if source_flag else (y[0] + y[1]) / 2
        loss = criterion(output, label)
        pred = torch.max(output, 1)[1]
        if per_class:
            for c in np.unique(label.cpu().numpy()):
                rows = label == int(c)
                k = int(pred[rows].eq(label[rows]).sum().cpu())
                acc[c, 0] += k / float(int(rows.sum().cpu()))
                acc[c, 1] += 1
        ratios.append(int(pred.eq(label).sum().cpu()) / float(data.shape[0]))
        loss_sum += loss.item() * data.shape[0]
        hits = hits + torch.sum(pred == label)
        n_rows += data.shape[0]
    pred_acc = hits.double() / n_rows
    with np.errstate(invalid='ignore', divide='ignore'):
        acc[:, 2] = acc[:, 0] / acc[:, 1]
    if pred_acc > best:
        best, best_epoch = pred_acc, epoch
    return {'cur_target_acc': pred_acc, 'best_target_acc': best, 'best_target_acc_epoch': best_epoch,
            'class_acc': acc, 'class_acc_mean': np.mean(acc[:, 2]), 'instance_acc': np.mean(ratios),
            'pred_loss': loss_sum / n_rows}


def _eval_dict(model, batches, criterion, num_class=10, source_flag=False, cls_eval=True, epoch=0):
    d = {'model': model, 'dataloader': batches, 'dataset': 'test1', 'best_target_acc': 0.0, 'device': torch.device('cuda:0'),
         'criterion': criterion, 'epoch': epoch, 'best_target_acc_epoch': 0, 'dataset_name': 'synthetic',
         'num_class': num_class, 'cls_eval': cls_eval}
    if source_flag:
        d['source_flag'] = True
    return d


def _compare(res, ref):
    from sug_amd.utils.eval_utils import LAST
    assert res['cur_target_acc'].dtype == torch.float64 and res['cur_target_acc'].dim() == 0
    assert torch.equal(res['cur_target_acc'], ref['cur_target_acc'])
    assert torch.equal(torch.as_tensor(res['best_target_acc']).cpu(), torch.as_tensor(ref['best_target_acc']).cpu())
    assert res['best_target_acc_epoch'] == ref['best_target_acc_epoch']
    np.testing.assert_array_equal(LAST['class_acc'], ref['class_acc'])          # NaN positions included
    assert LAST['instance_acc'] == ref['instance_acc']
    assert np.array_equal(LAST['class_acc_mean'], ref['class_acc_mean'], equal_nan=True)
    assert abs(LAST['pred_loss'] - ref['pred_loss']) <= 1e-6 * max(1.0, abs(ref['pred_loss']))


# ------------------------------------------------------------------ 1. the kernel against torch
def case_kernel_against_torch_and_graph_capture():
    from sug_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(7)
    for C in (10, 40):
        state = ops.eval_state(8, dev)
        class_acc = np.zeros((C, 2))
        ratios, loss_total, correct_total, rows_c, corr_c = [], 0.0, 0, np.zeros(C, np.int64), np.zeros(C, np.int64)
        batches = []
        for B in (1, 7, 32, 333):
            a = torch.randint(-3, 4, (B, C), generator=g).float()           # small integers: exact ties
            b = torch.randint(-3, 4, (B, C), generator=g).float()
            if B >= 7:
                a[1], b[1] = 2.0, 2.0                                          # a row of equal values
                a[2, 3] = float('nan')                                         # a NaN row
                a[4] += torch.randn(C, generator=g)
            lab = torch.randint(0, C - 1, (B,), generator=g)                   # class C-1 never present
            batches.append((a.to(dev), b.to(dev), lab.to(dev)))
        ce = nn.CrossEntropyLoss()
        for a, b, lab in batches:
            B = a.shape[0]
            out = torch.empty(B, C, device=dev)
            pred = torch.empty(B, dtype=torch.int64, device=dev)
            ops.eval_accumulate(state, a, lab, logits2=b, ce=('mean', -100, 0.0), out=out, pred=pred, cls_eval=True)
            output = (a + b) / 2
            assert torch.equal(out, output) or torch.equal(out.isnan(), output.isnan()) and \
                torch.equal(out.nan_to_num(), output.nan_to_num())
            tp = torch.max(output, 1).indices
            assert torch.equal(pred, tp), 'argmax differs from torch.max'
            p, y = tp.cpu().numpy(), lab.cpu().numpy()
            for c in np.unique(y):
                sel = y == c
                class_acc[c, 0] += int((p[sel] == c).sum()) / float(int(sel.sum()))
                class_acc[c, 1] += 1
                rows_c[c] += int(sel.sum())
                corr_c[c] += int((p[sel] == c).sum())
            k = int((p == y).sum())
            ratios.append(k / float(B))
            correct_total += k
            loss_total += ce(output, lab).item() * B
        f = ops.eval_state_fields(state)
        assert f['error'] == 0 and f['batch_count'] == 4 and f['data_total'] == 373
        assert f['correct_total'] == correct_total
        np.testing.assert_array_equal(f['class_rows'][:C], rows_c)
        np.testing.assert_array_equal(f['class_correct'][:C], corr_c)
        np.testing.assert_array_equal(f['class_acc'][:C], class_acc)
        assert not f['class_acc'][C:].any()
        assert f['batch_acc'].tolist() == ratios
        if np.isnan(loss_total):
            assert np.isnan(f['loss_total'])
        else:
            assert abs(f['loss_total'] - loss_total) <= 1e-6 * abs(loss_total)

        # the same launches captured into a graph and replayed
        st2 = ops.eval_state(8, dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ops.capture_guard(), torch.cuda.graph(graph):
            for a, b, lab in batches:
                ops.eval_accumulate(st2, a, lab, logits2=b, ce=('mean', -100, 0.0), cls_eval=True)
        st2.zero_()
        graph.replay()
        f2 = ops.eval_state_fields(st2)
        for k in ('batch_count', 'data_total', 'correct_total', 'error'):
            assert f2[k] == f[k], k
        for k in ('class_acc', 'class_rows', 'class_correct', 'batch_acc'):
            np.testing.assert_array_equal(f2[k], f[k])
        assert f2['loss_total'] == f['loss_total'] or (np.isnan(f2['loss_total']) and np.isnan(f['loss_total']))
        del graph

    # a label outside [0, C) sets the error word (no device assert), a caller loss scalar is used as given
    st = ops.eval_state(1, dev)
    a = torch.randn(5, 10, device=dev)
    ops.eval_accumulate(st, a, torch.tensor([0, 1, 12, 3, 4], device=dev), loss=torch.tensor(0.5, device=dev))
    f = ops.eval_state_fields(st)
    assert f['error'] & 1 and f['loss_total'] == 2.5


# ------------------------------------------------------------------ 2./3. end to end
def _model(kind):
    from sug_amd.model.Model import Net_MDA
    from sug_amd.model.model_pointnet import Pointnet_cls
    net = Pointnet_cls() if kind == 'Pointnet_cls' else Net_MDA(kind)
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 3))
    return net.cuda()


SIZES = {'DGCNN': (6, 1024), 'Pointnet': (8, 1024), 'Pointnet2': (4, 2048), 'PTran': (2, 1024), 'Pointnet_cls': (8, 1024)}


def _setup(kind, seed=5):
    B, N = SIZES[kind]
    g = torch.Generator().manual_seed(seed)
    net = _model(kind).train()
    torch.manual_seed(seed)
    with torch.no_grad():
        net(O.synth_clouds(B, N, g).cuda())                                     # BatchNorm running buffers
    net.eval()
    batches = []
    for b in (B, B, B, max(1, B // 2)):                                          # three full batches and a partial one
        batches.append((O.synth_clouds(b, N, g).cuda(), torch.randint(0, 9, (b,), generator=g).cuda()))   # class 9 unseen
    return net, batches


def _epoch(net, batches, criterion, seed, **kw):
    from sug_amd.utils.eval_utils import eval_worker
    torch.manual_seed(seed)
    with torch.no_grad():
        ref = restated_loop(copy.deepcopy(net), batches, criterion, 10, kw.get('source_flag', False), kw.get('cls_eval', True))
    rng_ref = torch.get_rng_state()
    torch.manual_seed(seed)
    with torch.no_grad():
        res = eval_worker(_eval_dict(copy.deepcopy(net), batches, criterion, **kw), LOG)
    assert torch.equal(torch.get_rng_state(), rng_ref), 'the CPU generator stream differs from the eager loop'
    return res, ref


def case_eval_worker_two_epochs_equal_the_eager_loop(kind):
    from sug_amd import eval_graphs
    from sug_amd.utils.eval_utils import LAST
    net, batches = _setup(kind)
    source_flag = kind == 'Pointnet_cls'
    ce = nn.CrossEntropyLoss().cuda()
    res, ref = _epoch(net, batches, ce, 11, source_flag=source_flag)
    _compare(res, ref)
    assert LAST['form'] == 'device' and LAST['graphs'] and LAST['syncs'] == 1
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.01 * torch.randn_like(p))                                   # the next epoch's weights
    runner = eval_graphs.runner_for(net)
    before = dict(runner.stats)
    res, ref = _epoch(net, batches, ce, 12, source_flag=source_flag)
    _compare(res, ref)
    # epoch 2: every batch replays, the partial one included (captured now)
    assert runner.stats['replayed'] - before['replayed'] == 4, runner.stats
    assert runner.stats['eager'] == before['eager'] and runner.stats['refused'] == 0, (runner.stats, runner.why)


def case_fallbacks_give_identical_results():
    from sug_amd import eval_graphs
    from sug_amd.model.model_utils import focal_loss
    from sug_amd.utils.eval_utils import LAST
    net, batches = _setup('Pointnet')
    # model left in train mode: eager calls (dropout off, so the comparison is exact)
    for m in net.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d)):
            m.p = 0.0
    net.train()
    n0 = eval_graphs.FALLBACKS['train mode']
    res, ref = _epoch(net, batches, nn.CrossEntropyLoss(), 21)
    _compare(res, ref)
    assert eval_graphs.FALLBACKS['train mode'] == n0 + 1 and not LAST['graphs']
    net.eval()
    # focal_loss: called once per batch on the averaged logits; its alpha as after the eager loop
    fl_ref, fl = focal_loss(gamma=2, num_classes=10), focal_loss(gamma=2, num_classes=10)
    torch.manual_seed(22)
    with torch.no_grad():
        ref = restated_loop(copy.deepcopy(net), batches, fl_ref, 10, False, True)
    from sug_amd.utils.eval_utils import eval_worker
    torch.manual_seed(22)
    with torch.no_grad():
        res = eval_worker(_eval_dict(copy.deepcopy(net), batches, fl), LOG)
    _compare(res, ref)
    assert LAST['form'] == 'device' and LAST['pred_loss'] == ref['pred_loss']
    assert torch.equal(fl.alpha.cpu(), fl_ref.alpha.cpu())
    # cls_eval=False: no per-class ratios (all NaN)
    res, ref = _epoch(net, batches, nn.CrossEntropyLoss(), 23, cls_eval=False)
    _compare(res, ref)
    assert np.isnan(LAST['class_acc'][:, 2]).all()


# ------------------------------------------------------------------ 4. refreshed weights reach the replays
def case_replays_see_weights_after_training_steps():
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    from sug_amd.utils.eval_utils import LAST
    B, N = 4, 1024
    g = torch.Generator().manual_seed(31)
    net = Net_MDA('DGCNN')
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 4))
    torch.manual_seed(31)
    tr = SUGStep(net.cuda().train(), use_graph=False, share_prefix=True)
    assert any(getattr(m, 'cache_weight_split', False) for m in net.modules())
    data, data_t = O.synth_clouds(B, N, g).cuda(), O.synth_clouds(B, N, g).cuda()
    label, label_t = torch.randint(0, 10, (B,), generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()
    batches = [(O.synth_clouds(B, N, g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()) for _ in range(3)]
    ce = nn.CrossEntropyLoss()
    for rnd in range(2):
        tr.step(data, label, data_t, label_t)
        snap = copy.deepcopy(net).eval()
        res, ref = _epoch(snap, batches, ce, 40 + rnd)
        _compare(res, ref)
        assert LAST['graphs']


CASES = [('kernel_against_torch_and_graph_capture', case_kernel_against_torch_and_graph_capture, ())] + \
    [('eval_worker_two_epochs_equal_the_eager_loop[%s]' % k, case_eval_worker_two_epochs_equal_the_eager_loop, (k,)) for k in KINDS] + \
    [('fallbacks_give_identical_results', case_fallbacks_give_identical_results, ()),
     ('replays_see_weights_after_training_steps', case_replays_see_weights_after_training_steps, ())]


def main(out_path):
    from sug_amd.model.Model import Net_MDA
    Net_MDA.call_graphs = False             # the form tests/conftest.py pins for every test
    res = {}
    for name, fn, args in CASES:
        try:
            fn(*args)
            res[name] = None
        except Exception:
            res[name] = traceback.format_exc()
        with open(out_path, 'w') as fh:     # after every case: a crash leaves the results so far
            json.dump(res, fh)


if __name__ == '__main__':
    main(sys.argv[1])
