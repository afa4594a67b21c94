"""GPU: model/dgcnn_seg.DGCNNPartSeg at B = 2, N = 128, k = 20, emb_dims 256, 50 parts, 16 categories against the
restatement of tests/dgcnn_seg_cases.py on the CPU, and the training / evaluation plumbing around it (SegStep,
seg_eval_worker, DeviceLoader(PartSegDataset)) unchanged.

Teacher-forced runs (the four neighbour lists given, taken from the fp64 restatement's own free run) compare logits, the
global feature, every BatchNorm buffer and every parameter gradient under the project's bound: err(t) = max|t - ref64| /
max|ref64|, err(model) <= 8 err(the restatement in fp32 torch) + 1e-7; each tensor's two figures are printed as
`dgcnn-seg-ratio model-<mode> <tensor> ...` before the assertion.  Their input is dgcnn_seg_cases.find_inputs': the first
draw whose fp64 forward keeps every pre-activation off the kink of its LeakyReLU / ReLU and every max off a tie by a stated
margin -- one element on the other side of a kink moves a 256-row BatchNorm-bias gradient by 1e-2 (seen on the first draw in
train mode with the input transform), which says nothing about either side's arithmetic.  Measured on an MI355X
(profiles/dgcnn_seg_fp64_ratios.txt): the worst err(model) / (err(fp32 torch) + 1e-7 / 8) is 4.46 (d transform_net.fc3.weight,
train), the T-Net's and conv7's gradients sit at 3.2 .. 3.9, everything else lower; the bound holds up to 8."""
import hashlib

import numpy as np
import pytest
import torch

import dgcnn_seg_cases as D
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu


def _cls():
    from sug_amd.model.dgcnn_seg import DGCNNPartSeg
    return DGCNNPartSeg


def _ref_name(n):
    """The model registers bnK before convK: named_parameters() calls convK's BatchNorm bnK.*; the restatement convK.1.*"""
    head, _, rest = n.partition('.')
    return 'conv%s.1.%s' % (head[2:], rest) if head.startswith('bn') and head[2:].isdigit() else n


def _sd_cpu(net):
    return {n: t.detach().cpu().clone() for n, t in net.state_dict().items()}


def _hip_run(net, graphs=None, seed=D.MODEL_SEED):
    from sug_amd import ops
    pts, cat, lab = D.model_inputs(seed)
    g32 = None if graphs is None else [None if g is None else g.to(torch.int32).cuda() for g in graphs]
    logits, feat, used = net(pts.cuda(), cat.cuda(), knn_idx=g32, return_graphs=True)
    loss = ops.point_ce(logits, lab.cuda())
    loss.backward()
    torch.cuda.synchronize()
    grads = {_ref_name(n): (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu() for n, p in net.named_parameters()}
    buffers = {n: t.detach().cpu() for n, t in net.state_dict().items() if 'running_' in n and not n.startswith('bn')}
    return {'logits': logits.detach().cpu(), 'feat': feat.detach().cpu(), 'loss': float(loss.detach()), 'grads': grads, 'buffers': buffers,
            'graphs': [None if u is None else u.cpu().long() for u in used]}


def _compare(tag, res, r64, r32, train):
    assert set(res['grads']) == set(r64['names']), set(res['grads']) ^ set(r64['names'])
    names = list(r64['names'])
    # A constant added in front of train-mode batch statistics has a gradient of exactly zero: the biases of the T-Net's
    # convolutions, and bn6's bias where every cloud's pooled maximum sits on the same side of the activation (the per-cloud
    # columns of conv8 then move by one constant, which bn8 removes).  The fp64 reference of such a tensor is rounding noise
    # (below 1e-10 here; the true gradients are 1e-3 and more), the relative error means nothing, and the tensor is held
    # against 1e-4 of the largest gradient of the run instead: fp32 cancellation noise over these 256 rows / 5120 edges is
    # some 1e-6 of the terms it sums, a wrong gradient is of their order.
    top = max(float(r64['grads'][n].abs().max()) for n in names)
    for n in [n for n in names if float(r64['grads'][n].abs().max()) < 1e-10]:
        assert train, n
        names.remove(n)
        print('dgcnn-seg-zero %s %s %.4g (fp32 torch %.4g)' % (tag, n, float(res['grads'][n].abs().max()), float(r32['grads'][n].abs().max())))
        assert float(res['grads'][n].abs().max()) <= 1e-4 * max(1.0, top), (n, float(res['grads'][n].abs().max()))
    pairs = [('logits', res['logits'], r64['logits'], r32['logits']), ('feat', res['feat'], r64['feat'], r32['feat']),
             ('loss', torch.tensor(res['loss']), torch.tensor(r64['loss']), torch.tensor(r32['loss']))]
    pairs += [(n, res['buffers'][n], r64['buffers'][n], r32['buffers'][n]) for n in sorted(r64['buffers'])]
    pairs += [('d ' + n, res['grads'][n], r64['grads'][n], r32['grads'][n]) for n in names]
    bad = {}
    for n, got, a, b in pairs:
        ek, e32 = D.err(got, a), D.err(b, a)
        print('dgcnn-seg-ratio %s %s %.4g %.4g' % (tag, n.replace(' ', ''), ek, e32))
        assert tuple(got.shape) == tuple(a.shape) and bool(torch.isfinite(got).all()), n
        if not D.within(ek, e32):
            bad[n] = (ek, e32)
    assert not bad, '%s: err(model), err(fp32 torch) = %r' % (tag, bad)


@pytest.mark.parametrize('mode, transform', [('train', True), ('eval', True), ('train', False)])
def test_teacher_forced_against_fp64(mode, transform):
    train = mode == 'train'
    net = D.build_model(_cls(), 0.0, transform).train(train)
    sd = _sd_cpu(net)
    # an input that keeps every activation off its kink and every max off a tie, and the restatement's own lists on it
    seed, graphs, draws = D.find_inputs(sd, train, transform)
    print('dgcnn-seg-input model-%s%s seed %d (draw %d)' % (mode, '' if transform else '-notransform', seed, draws))
    r64 = D.run_reference(sd, torch.float64, train, transform, graphs, seed)
    r32 = D.run_reference(sd, torch.float32, train, transform, graphs, seed)
    res = _hip_run(net.cuda(), graphs, seed)
    m = D.MODEL
    assert res['logits'].shape == (m['B'], m['N'], m['num_part']) and res['feat'].shape == (m['B'], m['emb_dims'])
    for i, u in enumerate(res['graphs']):
        assert (u is None) if (i == 0 and not transform) else torch.equal(u, graphs[i])
    if train:
        assert int(net.bn1.num_batches_tracked) == 1 and int(net.bn10.num_batches_tracked) == 1
    _compare('model-%s%s' % (mode, '' if transform else '-notransform'), res, r64, r32, train)


def test_free_running_graphs_and_the_restatement_on_them():
    net = D.build_model(_cls(), 0.0, True).train()
    with torch.no_grad():                                       # the initial transform: fc3 = 0, T = identity
        net.transform_net.fc3.weight.zero_(), net.transform_net.fc3.bias.zero_()
    sd = _sd_cpu(net)
    res = _hip_run(net.cuda())
    pts = D.model_inputs()[0]
    want = O.knn_idx(pts, D.MODEL['k'])
    assert torch.equal(res['graphs'][0], want) and torch.equal(res['graphs'][1], want), 'the xyz graphs equal the oracle exactly'
    for u in res['graphs']:
        assert u.shape == (D.MODEL['B'], D.MODEL['N'], D.MODEL['k']) and int(u.min()) >= 0 and int(u.max()) < D.MODEL['N']
    r64 = D.run_reference(sd, torch.float64, True, True, res['graphs'])
    r32 = D.run_reference(sd, torch.float32, True, True, res['graphs'])
    for n in ('logits', 'feat'):
        ek, e32 = D.err(res[n], r64[n]), D.err(r32[n], r64[n])
        print('dgcnn-seg-ratio model-free %s %.4g %.4g' % (n, ek, e32))
        assert D.within(ek, e32), (n, ek, e32)


def test_input_checks():
    net = D.build_model(_cls()).cuda()
    cat = torch.zeros(2, dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError, match=r'\[B,3,N\]'):
        net(torch.zeros(2, 6, 64, device='cuda'), cat)
    with pytest.raises(RuntimeError, match='fewer than k'):
        net(torch.zeros(2, 3, 19, device='cuda'), cat)
    with pytest.raises(RuntimeError, match='category int64'):
        net(torch.zeros(2, 3, 64, device='cuda'), cat.int())
    with pytest.raises(RuntimeError, match='category int64'):
        net(torch.zeros(2, 3, 64, device='cuda'), torch.zeros(3, dtype=torch.int64, device='cuda'))
    with pytest.raises(RuntimeError, match='HIP device'):
        net(torch.zeros(2, 3, 64), cat)
    with pytest.raises(RuntimeError, match='HIP device'):
        net(torch.zeros(2, 3, 64, device='cuda'), cat.cpu())
    with pytest.raises(RuntimeError, match='fp32'):
        net(torch.zeros(2, 3, 64, device='cuda', dtype=torch.float16), cat)
    with pytest.raises(RuntimeError, match='knn_idx'):
        net(torch.zeros(2, 3, 64, device='cuda'), cat, knn_idx=[torch.zeros(2, 64, 20, dtype=torch.int64, device='cuda')] * 4)
    # a category outside the range gives a zero one-hot row, no fault
    with torch.no_grad():
        pts = D.model_inputs()[0].cuda()
        logits, _ = net.eval()(pts, torch.tensor([99, -3], device='cuda'))
    assert bool(torch.isfinite(logits).all())


def _three_steps():
    from sug_amd.seg_step import SegStep
    net = D.build_model(_cls(), dropout=0.5).cuda().train()
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    step = SegStep(net, lr=1e-3)
    step.set_epoch(1, 10)
    losses = []
    for s in range(3):
        pts, cat, lab = D.model_inputs(D.MODEL_SEED + s)
        losses.append(step.step(pts.cuda(), cat.cuda(), lab.cuda()))
    h = hashlib.sha256()
    for p in net.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    return step, net, [v.item() for v in losses], h.hexdigest()


def test_seg_step_is_reproducible_and_keeps_the_books():
    step, net, losses, digest = _three_steps()
    _, _, losses2, digest2 = _three_steps()
    assert losses == losses2 and digest == digest2, 'three steps from fixed seeds differ between two runs'
    assert all(np.isfinite(losses))
    loss_total, rows, correct = step.epoch_totals(reset=False)
    counts = [int((D.model_inputs(D.MODEL_SEED + s)[2] != -100).sum()) for s in range(3)]
    want = sum(float(np.float32(v)) * n for v, n in zip(losses, counts))
    assert rows == sum(counts) and abs(loss_total - want) <= 1e-12 * abs(want), (loss_total, want)
    assert 0 <= correct <= rows and correct == int(correct)
    assert step.epoch_totals() == (loss_total, rows, correct) and step.epoch_totals() == (0.0, 0.0, 0.0)


def test_seg_eval_worker():
    from sug_amd.utils.seg_utils import PartIoUMeter, seg_eval_worker
    m = D.MODEL
    net = D.build_model(_cls(), dropout=0.5).cuda().train()
    batches = [D.model_inputs(D.MODEL_SEED + s, ignore=False) for s in range(2)]
    out = seg_eval_worker(net, batches, PartIoUMeter(D.PART_FIRST, D.PART_COUNT, 'cuda'))
    assert net.training, 'the mode is put back'
    assert out['shapes'] == 2 * m['B'] and out['rows'] == 2 * m['B'] * m['N']
    assert np.isfinite(out['loss']) and np.isfinite(out['instance_miou']) and 0.0 <= out['instance_miou'] <= 1.0
    assert np.isfinite(out['class_miou']) and 0.0 <= out['accuracy'] <= 1.0


def test_device_loader_feeds_one_step():
    from sug_amd.data import PartSegDataset
    from sug_amd.data.dataloader import DeviceLoader
    from sug_amd.seg_step import SegStep
    m = D.MODEL
    N, B = m['N'], m['B']
    r = np.random.RandomState(5)
    lengths, cats = (150, 200, 128, 260), (0, 3, 10, 15)
    clouds = [r.uniform(-0.5, 0.5, (L, 3)).astype(np.float32) for L in lengths]                # xyz only: E = 0
    labels = [D.PART_FIRST[c] + r.randint(0, D.PART_COUNT[c], L) for L, c in zip(lengths, cats)]
    ds = PartSegDataset(clouds, labels, np.array(cats), D.PART_FIRST, D.PART_COUNT, num_points=N, aug=True, seed=2)
    assert ds.extra_channels == 0
    step = SegStep(D.build_model(_cls(), dropout=0.5).cuda().train(), lr=1e-3)
    losses = [step.step(*batch) for batch in DeviceLoader(ds, batch_size=B, shuffle=True)]
    assert len(losses) == 2 and all(np.isfinite(float(v)) for v in losses)
    assert step.epoch_totals()[1] == 2 * B * N
