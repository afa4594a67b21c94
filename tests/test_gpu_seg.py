"""GPU: part segmentation on HIP -- ops.point_ce (sug_point_ce_fwd / _bwd) against torch.nn.functional.cross_entropy in fp64,
ops.part_iou_accumulate against the numpy restatement of the ShapeNet-Part protocol (tests/test_seg_host.py holds that one to
hand-worked numbers), Pointnet2PartSeg against the restated model on the CPU in fp32 and fp64, and SegStep.

Bounds.  point_ce: the project's own for the same arithmetic (tests/test_gpu_loss.py): value rtol 2e-6 / atol 1e-7, gradient
rtol 1e-5 / atol 1e-7; the arg-max exact on logits whose top two entries are more than 1e-3 apart.  Part IoU: integer words
equal, the fp64 sums within 1e-12 relative (both sides are fp64 sums of at most SUG_SEG_MAX_CATEGORY_PARTS ratios per shape
and B shapes).  Model: the margins tests/test_gpu_pn2_msg_fp.py holds the composed network to -- FPS and ball-query indices
exact, logits and loss within 1e-4, gradients by its norm / probe rule against fp32 and
`err_hip <= 2 * err_ref32 + 1e-5 * |ref64|` against fp64 -- at seg_cases.MODEL_SEED, where the fp32 and fp64 reference runs
agree on every index list (asserted on the CPU when the references are built).

Measured on one MI355X: the 22 tests of this file take 4.4 s (the CPU reference runs of the model included), the slowest
1.6 s (two times three SegStep steps)."""
import hashlib

import numpy as np
import pytest
import torch

import seg_cases as S
from test_gpu_pn2_msg_fp import close, fp64_rule, grads_against_fp32

pytestmark = pytest.mark.gpu


def _R():
    from sug_amd import ops
    return ops.POINT_CE_BLOCK_ROWS


def _labels(M, Cn, seed):
    return torch.randint(0, Cn, (M,), generator=torch.Generator().manual_seed(seed + 1))


def _weight(Cn):
    return torch.rand(Cn, generator=torch.Generator().manual_seed(Cn)) + 0.25


def _check_ce(z_dev, lab, w, ignore_index=-100, scale=1.0):
    """point_ce forward + backward on z_dev (requires grad) against the fp64 oracle on the same values."""
    from sug_amd import ops
    loss, pred = ops.point_ce(z_dev, lab.cuda(), None if w is None else w.cuda(), ignore_index, want_pred=True)
    (g,) = torch.autograd.grad(loss * scale, z_dev)
    ref, gref = S.ce_oracle(z_dev, lab, w, ignore_index)
    print('M=%d C=%d: loss %.9g (fp64 %.12g), max grad err %.3e' % (lab.numel(), z_dev.shape[-1], loss.item(), ref.item(),
                                                                 (g.cpu().double() - gref * scale).abs().max().item()))
    torch.testing.assert_close(loss.cpu().double(), ref, rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(g.cpu().double(), gref * scale, rtol=1e-5, atol=1e-7)
    assert pred.dtype == torch.int32 and pred.shape == z_dev.shape[:-1]
    assert torch.equal(pred.cpu().long(), z_dev.detach().cpu().double().argmax(dim=-1))
    return loss, g


# ------------------------------------------------------------------------------------------------ point_ce
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('Cn', [2, 33, 50, 64])
def test_point_ce_against_the_fp64_oracle(Cn, weighted):
    R = _R()
    for M in (1, 63, 65, R - 1, R, R + 1, 2 * R + 1):
        z = S.margin_logits(M, Cn, seed=1000 * Cn + M).cuda().requires_grad_(True)
        _check_ce(z, _labels(M, Cn, M), _weight(Cn) if weighted else None, scale=1.7)


def test_point_ce_row_stride_and_leading_dimensions():
    from sug_amd import ops
    R = _R()
    M, Cn = R + 37, 50
    wide = torch.zeros(M, 64)
    wide[:, :Cn] = S.margin_logits(M, Cn, seed=5)
    wide[:, Cn:] = 50.0                                     # columns behind the row: never read
    wide = wide.cuda().requires_grad_(True)
    lab = _labels(M, Cn, 5)
    z = wide[:, :Cn]
    assert z.stride(0) == 64 and ops.point_ce_supported(z, lab.cuda())
    loss, pred = ops.point_ce(z, lab.cuda(), want_pred=True)
    (g,) = torch.autograd.grad(loss, wide)
    ref, gref = S.ce_oracle(z, lab)
    torch.testing.assert_close(loss.cpu().double(), ref, rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(g[:, :Cn].cpu().double(), gref, rtol=1e-5, atol=1e-7)
    assert float(g[:, Cn:].abs().sum()) == 0.0
    assert torch.equal(pred.cpu().long(), z.detach().cpu().argmax(dim=-1))
    # [B, N, C] logits and [B, N] labels: flattened, pred comes back as [B, N]
    z3 = S.margin_logits(6 * 50, 8, seed=6).view(6, 50, 8).cuda().requires_grad_(True)
    _check_ce(z3, _labels(300, 8, 6).view(6, 50), None)
    assert not ops.point_ce_supported(torch.zeros(4, 65, device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda'))
    assert not ops.point_ce_supported(torch.zeros(4, 1, device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda'))


def test_point_ce_tied_rows_give_the_lowest_index():
    from sug_amd import ops
    z = torch.zeros(5, 10)
    z[0, [3, 7]] = 2.0              # -> 3
    z[1, :] = -1.5                  # all equal -> 0
    z[2, [9]] = 1.0                 # -> 9
    z[3, [0, 9]] = 4.0              # -> 0
    z[4, [5, 6, 8]] = 0.5           # -> 5
    _, pred = ops.point_ce(z.cuda(), torch.tensor([0, 1, -100, 3, 4]).cuda(), want_pred=True)
    assert pred.tolist() == [3, 0, 9, 0, 5]                 # every row, the ignored one included


@pytest.mark.parametrize('weighted', [False, True])
def test_point_ce_label_semantics(weighted):
    """Scattered ignore_index rows, one whole workgroup's rows ignored, then an out-of-range label: NaN loss, NaN in that
    row's gradient only, zero gradient in the ignored rows."""
    from sug_amd import ops
    R = _R()
    M, Cn = 3 * R + 5, 33
    w = _weight(Cn) if weighted else None
    lab = _labels(M, Cn, 9)
    lab[[0, 17, R - 1, 2 * R, M - 1]] = -100                # scattered
    lab[R:2 * R] = -100                                     # the second workgroup's rows, all of them
    z = S.margin_logits(M, Cn, seed=9).cuda().requires_grad_(True)
    _, g = _check_ce(z, lab, w)
    ignored = (lab == -100).cuda()
    assert float(g[ignored].abs().sum()) == 0.0
    # another ignore_index
    lab7 = lab.clone()
    lab7[lab7 == 7] = 8
    lab7[lab7 == -100] = 7
    _check_ce(z, lab7, w, ignore_index=7)
    # every row ignored: 0 / 0, as torch
    assert torch.isnan(ops.point_ce(z, torch.full((M,), -100).cuda()))
    # out of range: -1 and C (neither is ignore_index)
    for bad in (-1, Cn):
        lab2 = lab.clone()
        lab2[2 * R + 3] = bad
        loss = ops.point_ce(z, lab2.cuda(), None if w is None else w.cuda())
        (g2,) = torch.autograd.grad(loss, z)
        assert torch.isnan(loss)
        assert bool(torch.isnan(g2[2 * R + 3]).all())
        others = torch.ones(M, dtype=torch.bool)
        others[2 * R + 3] = False
        assert not bool(torch.isnan(g2[others.cuda()]).any())
        assert float(g2[ignored].abs().sum()) == 0.0


def test_point_ce_totals_and_reproducibility():
    from sug_amd import ops
    R = _R()
    M, Cn = 2 * R + 1, 50
    z = S.margin_logits(M, Cn, seed=11).cuda().requires_grad_(True)
    lab = _labels(M, Cn, 11)
    lab[::7] = -100
    counting = int((lab != -100).sum())
    w = _weight(Cn).cuda()
    totals = torch.zeros(2, dtype=torch.float64, device='cuda')
    runs = []
    for _ in range(2):
        loss = ops.point_ce(z, lab.cuda(), w, totals=totals)
        (g,) = torch.autograd.grad(loss, z)
        runs.append((loss.clone(), g.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), 'not bit-reproducible'
    want = np.array([2 * float(runs[0][0].item()) * counting, 2.0 * counting])
    got = totals.cpu().numpy()
    assert got[1] == want[1] and abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (got, want)


# ------------------------------------------------------------------------------------------------ part IoU
def _state_books(state):
    from sug_amd import ops
    return ops.part_iou_state_fields(state)


def _same_books(got, want, what):
    K, Cn = len(S.PART_FIRST), S.NUM_PARTS
    for k in ('shapes', 'points', 'correct', 'error'):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got['cat_shapes'][:K].tolist() == want['cat_shapes'].tolist() and not got['cat_shapes'][K:].any(), what
    for k in ('part_points', 'part_correct'):
        assert got[k][:Cn].tolist() == want[k].tolist() and not got[k][Cn:].any(), (what, k)
    np.testing.assert_allclose(got['cat_iou'][:K], want['cat_iou'], rtol=1e-12, atol=0, err_msg=what)
    assert not got['cat_iou'][K:].any()


def _accumulate(state, z, lab, cat):
    from sug_amd import ops
    ops.part_iou_accumulate(torch.as_tensor(z).cuda(), torch.as_tensor(lab).cuda(), torch.as_tensor(cat).cuda(), S.PART_FIRST,
                            S.PART_COUNT, state)


def test_part_iou_against_the_restatement():
    from sug_amd import ops
    # B = 1, N = 1
    z, lab, cat = S.random_case(1, 1, seed=1, categories=[2])
    st = ops.part_iou_state('cuda')
    _accumulate(st, z, lab, cat)
    _same_books(_state_books(st), S.part_iou_books(z, lab, cat, S.PART_FIRST, S.PART_COUNT), 'B=1 N=1')
    # the hand-worked clouds: an absent part, ties, a maximum outside the range, the one-part category
    z, lab, cat = S.hand_case()
    st = ops.part_iou_state('cuda')
    _accumulate(st, z, lab, cat)
    got = _state_books(st)
    _same_books(got, S.part_iou_books(z, lab, cat, S.PART_FIRST, S.PART_COUNT), 'hand case')
    assert got['correct'] == 19 and got['cat_iou'][1] == 1.0 and got['cat_iou'][2] == 0.45
    # B = 3, N = 100 (no multiple of 64), the three categories; a column outside each range made the global maximum
    z, lab, cat = S.random_case(3, 100, seed=2, categories=[1, 2, 0])
    z[0, :, 0] = 30.0
    z[1, :, 2] = 30.0
    z[2, :, 5] = 30.0
    st2 = ops.part_iou_state('cuda')
    _accumulate(st2, z, lab, cat)
    want = S.part_iou_books(z, lab, cat, S.PART_FIRST, S.PART_COUNT)
    _same_books(_state_books(st2), want, 'B=3 N=100')
    # two calls accumulate: the state equals the restatement over the concatenated batches
    z2, lab2, cat2 = S.random_case(5, 300, seed=3)
    _accumulate(st2, z2, lab2, cat2)
    _same_books(_state_books(st2), S.part_iou_books(z2, lab2, cat2, S.PART_FIRST, S.PART_COUNT, want), 'two calls')


def test_part_iou_bad_clouds_are_counted_and_not_scored():
    from sug_amd import ops
    from sug_amd.utils.seg_utils import PartIoUMeter
    z, lab, cat = S.random_case(4, 70, seed=4, categories=[0, 2, 1, 0])
    good = S.part_iou_books(z[[0, 2]], lab[[0, 2]], cat[[0, 2]], S.PART_FIRST, S.PART_COUNT)
    lab[1, 33] = 3                                          # a label outside category 2's range {4, 5}
    cat[3] = len(S.PART_FIRST)                              # category == K
    meter = PartIoUMeter(S.PART_FIRST, S.PART_COUNT, 'cuda')
    meter.update(torch.as_tensor(z).cuda(), torch.as_tensor(lab).cuda(), torch.as_tensor(cat).cuda())
    got = _state_books(meter.state)
    assert got['error'] == 2
    good['error'] = 2
    _same_books(got, good, 'bad clouds')
    assert S.part_iou_books(z, lab, cat, S.PART_FIRST, S.PART_COUNT)['error'] == 2
    with pytest.raises(IndexError, match='not scored'):
        meter.result()
    meter.reset()
    assert not bool(meter.state.any())


def test_part_iou_meter_result():
    from sug_amd.utils.seg_utils import PartIoUMeter
    z, lab, cat = S.hand_case()
    meter = PartIoUMeter(S.PART_FIRST, S.PART_COUNT, 'cuda')
    meter.update(torch.as_tensor(z).cuda(), torch.as_tensor(lab).cuda(), torch.as_tensor(cat).cuda())
    r = meter.result()
    ious = [(0.6 + 0.6 + 1.0) / 3, 1.0, 0.45]
    assert r['shapes'] == 3 and r['category_shapes'].tolist() == [1, 1, 1]
    assert r['instance_miou'] == pytest.approx(sum(ious) / 3, rel=1e-12) and r['class_miou'] == pytest.approx(sum(ious) / 3, rel=1e-12)
    np.testing.assert_allclose(r['category_miou'], ious, rtol=1e-12)
    assert r['accuracy'] == 19 / 24
    # parts seen: 0, 1, 3, 4, 5 with accuracies 3/4, 3/4, 1, 1/2, 1
    assert r['part_avg_accuracy'] == pytest.approx((0.75 + 0.75 + 1.0 + 0.5 + 1.0) / 5, rel=1e-12)


# ------------------------------------------------------------------------------------------------ model
def _hip_run(mode, extra):
    from sug_amd import ops
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    net = S.build_model(Pointnet2PartSeg, extra, dropout=0.0 if mode == 'train' else 0.5).cuda().train(mode == 'train')
    res = S.run_model(net, S.model_inputs(extra), lambda y, lab: ops.point_ce(y, lab), device='cuda')
    return net, res


@pytest.mark.parametrize('mode, extra', [('train', 0), ('eval', 0), ('train', 3)])
def test_model_against_the_restatement(mode, extra):
    m = S.MODEL
    r32, r64, lists = S.reference_runs(mode, extra)
    net, res = _hip_run(mode, extra)
    assert res['logits'].shape == (m['B'], m['N'], m['num_part']) and res['feat'].shape == (m['B'], 1024)
    # the index half: sa1's FPS draw and ball-query lists, from the same generator state
    pts = S.model_inputs(extra)[0]
    torch.manual_seed(S.MODEL_SEED + 1)
    _, fps, bq = net.sa1.group_indices(pts[:, :3].permute(0, 2, 1).contiguous().cuda())
    assert torch.equal(fps.cpu().long(), lists[0]), 'FPS indices'
    for i, idx in enumerate(bq):
        assert torch.equal(idx.cpu().long(), lists[2 + i]), 'ball-query lists of scale %d' % i
    close(res['logits'], r32['logits'], 1e-4, '%s logits' % mode)
    close(res['feat'], r32['feat'], 1e-4, '%s global feature' % mode)
    assert abs(res['loss'] - r32['loss']) <= 1e-4 * max(1.0, abs(r32['loss'])), (res['loss'], r32['loss'])
    assert res['grad_names'] == r32['grad_names'] == r64['grad_names']
    norm, dot = np.array(res['grad_norm']), np.array(res['grad_dot'])
    gn32, gd32, gn64, gd64 = (np.array(v) for v in (r32['grad_norm'], r32['grad_dot'], r64['grad_norm'], r64['grad_dot']))
    grads_against_fp32('%s ' % mode, res['grad_names'], norm, dot, gn32, gd32, gn64, gd64)
    fp64_rule(norm, gn32, gn64, '%s gradient norms' % mode)
    fp64_rule(dot, gd32, gd64, '%s gradient probes' % mode)


def test_model_input_checks():
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    net = S.build_model(Pointnet2PartSeg).cuda()
    cat = torch.zeros(2, dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError, match='npoint1'):
        net(torch.zeros(2, 3, 32, device='cuda'), cat)
    with pytest.raises(RuntimeError, match='fp32'):
        net(torch.zeros(2, 3, 256, device='cuda', dtype=torch.float16), cat)
    with pytest.raises(RuntimeError, match=r'\[B,3,N\]'):
        net(torch.zeros(2, 6, 256, device='cuda'), cat)


# ------------------------------------------------------------------------------------------------ SegStep
def _three_steps():
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    from sug_amd.seg_step import SegStep
    net = S.build_model(Pointnet2PartSeg, dropout=0.5).cuda().train()
    torch.manual_seed(3)                                    # the FPS starts (CPU generator) and the dropout masks (device generator)
    torch.cuda.manual_seed(3)
    step = SegStep(net, lr=1e-3)
    step.set_epoch(1, 10)
    losses = []
    for s in range(3):
        pts, cat, lab = S.model_inputs(0, seed=S.MODEL_SEED + s)
        losses.append(step.step(pts.cuda(), cat.cuda(), lab.cuda()))
    h = hashlib.sha256()
    for p in net.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    return step, net, [v.item() for v in losses], h.hexdigest()


def test_seg_step_is_reproducible_and_keeps_the_books():
    from sug_amd import ops
    step, net, losses, digest = _three_steps()
    _, _, losses2, digest2 = _three_steps()
    assert losses == losses2 and digest == digest2, 'three steps from fixed seeds differ between two runs'
    assert all(np.isfinite(losses))
    loss_total, rows, correct = step.epoch_totals(reset=False)
    counts = [int((S.model_inputs(0, seed=S.MODEL_SEED + s)[2] != -100).sum()) for s in range(3)]
    want = sum(float(np.float32(v)) * n for v, n in zip(losses, counts))
    assert rows == sum(counts) and abs(loss_total - want) <= 1e-12 * abs(want), (loss_total, want)
    assert 0 <= correct <= rows and correct == int(correct)
    assert step.epoch_totals() == (loss_total, rows, correct) and step.epoch_totals() == (0.0, 0.0, 0.0)
    # correct points: one more step with the prediction recomputed on the host from the same forward (eval mode: no
    # dropout, the FPS draw repeated from the same generator state)
    pts, cat, lab = (t.cuda() for t in S.model_inputs(0, seed=S.MODEL_SEED + 5))
    net.eval()
    torch.manual_seed(21)
    with torch.no_grad():
        logits, _ = net(pts, cat)
    torch.manual_seed(21)
    loss = step.step(pts, cat, lab)
    lt, n, ok = step.epoch_totals()
    keep = (lab != -100).cpu()
    assert n == int(keep.sum()) and ok == int((logits.argmax(-1).cpu() == lab.cpu())[keep].sum())
    assert abs(lt - float(loss.item()) * n) <= 1e-12 * abs(lt)
    net.train()


def test_seg_eval_worker():
    from sug_amd import ops
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    from sug_amd.utils.seg_utils import PartIoUMeter, seg_eval_worker
    m = S.MODEL
    first, count = [0, 3, 5], [3, 2, 3]                     # three categories over the model case's eight parts
    net = S.build_model(Pointnet2PartSeg, dropout=0.5).cuda().train()
    batches = []
    for s in range(2):
        pts, cat, _ = S.model_inputs(0, seed=S.MODEL_SEED + s)
        g = torch.Generator().manual_seed(s)
        lab = torch.stack([first[k] + torch.randint(0, count[k], (m['N'],), generator=g) for k in cat.tolist()])
        batches.append((pts, cat, lab))
    meter = PartIoUMeter(first, count, 'cuda')
    torch.manual_seed(8)
    out = seg_eval_worker(net, batches, meter)
    assert net.training, 'the mode is put back'
    # the same forwards, the books on the host
    net.eval()
    torch.manual_seed(8)
    books, loss_total = None, 0.0
    with torch.no_grad():
        for pts, cat, lab in batches:
            logits, _ = net(pts.cuda(), cat.cuda())
            books = S.part_iou_books(logits.cpu().numpy(), lab.numpy(), cat.numpy(), first, count, books)
            loss_total += float(ops.point_ce(logits, lab.cuda()).item()) * lab.numel()
    assert out['shapes'] == books['shapes'] == 4 and out['rows'] == 4 * m['N']
    assert out['accuracy'] == books['correct'] / books['points']
    assert abs(out['instance_miou'] - books['cat_iou'].sum() / 4) <= 1e-12
    assert abs(out['loss'] - loss_total / out['rows']) <= 1e-12 * abs(out['loss'])
