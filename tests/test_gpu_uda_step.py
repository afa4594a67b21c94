"""GPU: the two-phase UDA / naive-MMD training step (sug_amd.uda_step.UDAStep) and its phase-1 loss kernel
(ops.mcd_loss = sug_mcd_loss_fwd / sug_mcd_loss_bwd).

  1. the kernel against torch in fp64 on the CPU (four outputs, gradients, determinism, sign(0) = 0, the books, the NaN contract);
  2. the orchestration against the reference's loop written out by hand, bit for bit;
  3. two steps against the CPU oracle, and the evidence that this comparison would see stale phase-2 weights (step 2 at the
     learning rate at which the oracle agrees with itself: _LR2);
  4. graph replay == eager launches, bit for bit, through a learning-rate change;
  5. fused loss + paired domains against the composed, unpaired form;  6. the epoch's books and the fallbacks."""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _logits(Ms, Mt, C, seed, ld=None):
    """Four logit blocks (as columns [:C] of wider tensors when ld is given), source labels and target labels; from 3 target rows
    on, rows 0 and 2 of the two target blocks hold EQUAL logits (the discrepancy's kink)."""
    g = torch.Generator().manual_seed(seed)
    wide = [torch.randn(M, ld or C, generator=g) * 3.0 for M in (Ms, Ms, Mt, Mt)]
    if Mt >= 3:
        wide[3][0] = wide[2][0]
        wide[3][2] = wide[2][2]
    return wide, torch.randint(0, C, (Ms,), generator=g), torch.randint(0, C, (Mt,), generator=g)


def _loss_of(zs, lab, lab_t, a_s, a_t, r_s):
    ces = F.cross_entropy(zs[0], lab) + F.cross_entropy(zs[1], lab)
    cet = (F.cross_entropy(zs[2], lab_t) + F.cross_entropy(zs[3], lab_t)) if a_t else torch.zeros((), dtype=zs[0].dtype, device=zs[0].device)
    D = torch.mean(torch.abs(F.softmax(zs[2], dim=-1) - F.softmax(zs[3], dim=-1)))
    loss = a_s * ces + a_t * cet - D
    return loss, torch.stack([loss.detach(), r_s * ces.detach(), -D.detach(), a_t * cet.detach()])


def _torch_run(zs, lab, lab_t, a_s, a_t, r_s, dtype, device):
    zs = [z.detach().to(device=device, dtype=dtype).clone().requires_grad_() for z in zs]
    loss, outs = _loss_of(zs, lab.to(device), lab_t.to(device), a_s, a_t, r_s)
    loss.backward()
    return outs.cpu().double(), [z.grad.cpu().double() for z in zs]


def _ours(zg, lab, lab_t, a_s, a_t, r_s, totals=None, paired=False):
    from sug_amd import ops
    zg = [z.detach().requires_grad_() for z in zg]
    if paired:
        out = ops.mcd_loss(zg[0], zg[1], None, None, lab, lab_t, a_s, a_t, r_s, totals=totals)
    else:
        out = ops.mcd_loss(zg[0], zg[1], zg[2], zg[3], lab, lab_t, a_s, a_t, r_s, totals=totals)
    out[0].backward()
    return torch.stack([o.detach() for o in out]), [z.grad for z in zg]


def _check_against_fp64(outs, grads, z64, lab, lab_t, a_s, a_t, r_s, tag):
    """The four outputs within 1e-4 * max(1, |ref|); per gradient block the error (relative L2 against fp64) <= 3 x that of the
    composed torch ops in fp32 on the same GPU + 1e-5 (the rule of tests/test_gpu_source_step.py)."""
    ref, g64 = _torch_run(z64, lab, lab_t, a_s, a_t, r_s, torch.float64, 'cpu')
    _, g32 = _torch_run(z64, lab, lab_t, a_s, a_t, r_s, torch.float32, DEV)
    got = outs.cpu().double()
    print('%s: outputs %s ref %s' % (tag, got.tolist(), ref.tolist()))
    for a, b in zip(got.tolist(), ref.tolist()):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (tag, got, ref)
    for i, (g, r, t) in enumerate(zip(grads, g64, g32)):
        n = max(float(r.norm()), 1e-30)
        e_gpu, e_ref = float((g.cpu().double() - r).norm()) / n, float((t - r).norm()) / n
        print('%s: block %d gradient error %.2e, torch fp32 %.2e' % (tag, i, e_gpu, e_ref))
        assert e_gpu <= 3.0 * e_ref + 1e-5, (tag, i, e_gpu, e_ref)


@pytest.mark.parametrize('a_t', [0.0, 0.25])
@pytest.mark.parametrize('C', [2, 10, 64])
@pytest.mark.parametrize('M', [1, 3, 65, 128])
def test_mcd_loss_against_fp64(M, C, a_t):
    a_s, r_s = 0.7, 0.5
    z, lab, _ = _logits(M, M, C, 1000 * M + C)
    lab_t = lab                                             # the step scores the target rows against the source labels
    zg, lg = [t.to(DEV) for t in z], lab.to(DEV)
    outs, grads = _ours(zg, lg, lg if a_t else None, a_s, a_t, r_s)
    outs_b, grads_b = _ours(zg, lg, lg if a_t else None, a_s, a_t, r_s)
    assert torch.equal(outs, outs_b) and all(torch.equal(a, b) for a, b in zip(grads, grads_b))      # two runs, bit for bit
    _check_against_fp64(outs, grads, z, lab, lab_t, a_s, a_t, r_s, 'M=%d C=%d a_t=%g' % (M, C, a_t))
    assert all(g.shape == (M, C) for g in grads)
    if M >= 3 and a_t == 0.0:                               # equal logits: sign(0) = 0, an exactly zero discrepancy gradient
        for r in (0, 2):
            assert float(grads[2][r].abs().max()) == 0.0 and float(grads[3][r].abs().max()) == 0.0
        assert float(grads[2][1].abs().max()) > 0.0
    if a_t == 0.0:
        assert float(outs[3]) == 0.0


@pytest.mark.parametrize('a_t', [0.0, 0.25])
def test_mcd_loss_strided_paired_layout(a_t):
    """ld = 48 > C = 40, and the paired layout: two [2M, 48] tensors whose column slices [:, :40] hold the source rows first --
    what Net_MDA.forward_pair(paired_out=True) returns; the gradient comes back as two dense [2M, 40] tensors."""
    M, C, a_s, r_s = 65, 40, 1.0, 1.0
    z, lab, _ = _logits(M, M, C, 77, ld=48)
    w1, w2 = torch.cat((z[0], z[2])).to(DEV), torch.cat((z[1], z[3])).to(DEV)
    y1, y2 = w1[:, :C], w2[:, :C]
    assert y1.stride(0) == 48 and y1.shape == (2 * M, C)
    lg = lab.to(DEV)
    outs, grads = _ours([y1, y2], lg, lg if a_t else None, a_s, a_t, r_s, paired=True)
    outs_b, grads_b = _ours([y1, y2], lg, lg if a_t else None, a_s, a_t, r_s, paired=True)
    assert torch.equal(outs, outs_b) and all(torch.equal(a, b) for a, b in zip(grads, grads_b))
    assert all(g.shape == (2 * M, C) and g.is_contiguous() for g in grads)
    blocks = [grads[0][:M], grads[1][:M], grads[0][M:], grads[1][M:]]
    _check_against_fp64(outs, blocks, [t[:, :C] for t in z], lab, lab, a_s, a_t, r_s, 'paired ld=48 a_t=%g' % a_t)
    # the same numbers from four separate (contiguous) blocks: the layout changes nothing, bit for bit
    outs_c, grads_c = _ours([t[:, :C].contiguous().to(DEV) for t in z], lg, lg if a_t else None, a_s, a_t, r_s)
    assert torch.equal(outs, outs_c) and all(torch.equal(a, b) for a, b in zip(blocks, grads_c))


def test_mcd_loss_unequal_row_counts():
    """Ms = 3 source rows, Mt = 7 target rows (a partial last batch of one loader): supported without the target cross entropy."""
    from sug_amd import ops
    z, lab, lab_t = _logits(3, 7, 10, 5)
    zg = [t.to(DEV) for t in z]
    assert ops.mcd_loss_supported(*zg, label=lab.to(DEV), a_t=0.0) and not ops.mcd_loss_supported(*zg, label=lab.to(DEV), a_t=0.25)
    outs, grads = _ours(zg, lab.to(DEV), None, 1.0, 0.0, 1.0)
    _check_against_fp64(outs, grads, z, lab, lab_t, 1.0, 0.0, 1.0, 'Ms=3 Mt=7')
    wide = torch.zeros(4, 65, device=DEV)
    assert not ops.mcd_loss_supported(wide, wide, wide, wide)                   # C = 65
    assert not ops.mcd_loss_supported(*[t.half() for t in zg])                  # not fp32


def test_mcd_loss_books_accumulate_in_the_same_launch():
    totals = torch.zeros(4, dtype=torch.float64, device=DEV)
    want = [0.0, 0.0, 0.0, 0.0]
    for M in (3, 65, 128):
        z, lab, _ = _logits(M, M, 10, M)
        outs, _ = _ours([t.to(DEV) for t in z], lab.to(DEV), None, 1.0, 0.0, 0.5, totals=totals)
        want[0] += float(outs[1]) * M                       # loss_total += loss_s.item() * data.size(0)
        want[1] += float(outs[2]) * M                       # loss_adv_total += loss_adv.item() * data.size(0)
        want[2] += M
        want[3] += M
    got = totals.tolist()
    assert got[2:] == want[2:]
    for a, b in zip(got[:2], want[:2]):
        assert abs(a - b) <= 4 * np.finfo(np.float64).eps * abs(b), (got, want)


def test_mcd_loss_out_of_range_labels_poison_the_loss():
    z, lab, _ = _logits(5, 5, 10, 9)
    zg = [t.to(DEV) for t in z]
    for bad in (10, -1):                                    # torch raises; the kernel poisons the result
        yb = lab.clone()
        yb[3] = bad
        outs, grads = _ours(zg, yb.to(DEV), None, 1.0, 0.0, 1.0)
        assert torch.isnan(outs[0]) and torch.isnan(outs[1]) and not torch.isnan(outs[2])
        assert torch.isnan(grads[0][3]).all() and torch.isnan(grads[1][3]).all()
        assert not torch.isnan(grads[0][[0, 1, 2, 4]]).any() and not torch.isnan(grads[2]).any()
        outs, grads = _ours(zg, lab.to(DEV), yb.to(DEV), 1.0, 0.25, 1.0)       # ... in the target rows' labels
        assert torch.isnan(outs[0]) and torch.isnan(outs[3]) and not torch.isnan(outs[1])
        assert torch.isnan(grads[2][3]).all() and not torch.isnan(grads[2][[0, 1, 2, 4]]).any() and not torch.isnan(grads[0]).any()


# ------------------------------------------------------------------------------------------------ models and runs
def _net(name, seed=3):
    from sug_amd.model.Model import Net_MDA
    net = Net_MDA(name)
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
    for m in net.modules():
        if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)):
            m.p = 0.0
    return net.to(DEV).train()


_BATCHES = {}


def _batches(B=4, N=1024):
    """Two fixed batches (source clouds, labels, target clouds, labels) on the host, made once and never written to."""
    if (B, N) not in _BATCHES:
        g = torch.Generator().manual_seed(17)
        _BATCHES[(B, N)] = [(O.synth_clouds(B, N, g), torch.randint(0, 10, (B,), generator=g),
                             O.synth_clouds(B, N, g), torch.randint(0, 10, (B,), generator=g)) for _ in range(2)]
    return _BATCHES[(B, N)]


def _sha(net):
    h = hashlib.sha256()
    for k, v in net.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def _schedule(steps, partial_every=3, B=4):
    """(batch index, rows) per step: two alternated batches, a partial batch of B - 1 rows every `partial_every`-th step."""
    return [(i % 2, B - 1 if (partial_every and i % partial_every == partial_every - 1) else B) for i in range(steps)]


def _run(name, steps=8, partial_every=3, hashes=True, epoch_at=None, **kw):
    from sug_amd.uda_step import UDAStep
    net = _net(name)
    tr = UDAStep(net, **kw)
    torch.manual_seed(11)
    losses, shas, sched = [], [], _schedule(steps, partial_every)
    for i, (bi, rows) in enumerate(sched):
        if epoch_at is not None and i == epoch_at:
            lrs = tr.set_epoch(7, 20)                       # all three rates change (cosine for g and c, one halving for dis)
            assert lrs[0] < tr.base_lr and lrs[1] < tr.c_lr and lrs[2] == 0.5 * tr.base_lr * tr.lr_scaler
        x, lab, xt, lab_t = (t[:rows].to(DEV) for t in _batches()[bi])
        losses.append(torch.stack(tr.step(x, lab, xt, lab_t)))
        if hashes:
            shas.append(_sha(net))
    return {'losses': torch.stack(losses).cpu(), 'shas': shas, 'rng': torch.get_rng_state(), 'tr': tr, 'net': net,
            'rows': [r for _, r in sched]}


# ------------------------------------------------------------------------------------------------ 2. the orchestration
def _literal_loop(name, recipe, steps, lr=1e-3, weight_decay=5e-5, scaler=1.0, weight=1.0, target_loss=1.0):
    """train_uda.py:101-113, :149-178 / train_dg_naive_mmd.py:174-186, :225-257, line by line, on the same Net_MDA."""
    from sug_amd.model import mmd
    from sug_amd.train_step import discrepancy
    from sug_amd.uda_step import CLASS_MMD
    model = _net(name)
    model.call_graphs = False                               # the literal caller launches every call from Python
    criterion = torch.nn.CrossEntropyLoss()
    params = [{'params': v} for k, v in model.g.named_parameters() if 'pred_offset' not in k]
    optimizer_g = torch.optim.Adam(params, lr=lr, weight_decay=weight_decay)
    optimizer_c = torch.optim.Adam([{'params': model.c1.parameters()}, {'params': model.c2.parameters()}],
                                   lr=lr * 2 if recipe == 'uda' else lr, weight_decay=weight_decay)
    optimizer_dis = torch.optim.Adam([{'params': model.g.parameters()}, {'params': model.attention_s.parameters()},
                                      {'params': model.attention_t.parameters()}], lr=lr * scaler, weight_decay=weight_decay)
    cons = 1.0
    torch.manual_seed(11)
    losses, shas = [], []
    for bi, rows in _schedule(steps, 0):
        data, label, data_t, label_t = (t[:rows].to(DEV) for t in _batches()[bi])
        pred_s1, pred_s2 = model(data)
        pred_t1, pred_t2 = model(data_t, constant=cons, adaptation=True)
        loss_s1 = criterion(pred_s1, label)
        loss_s2 = criterion(pred_s2, label)
        loss_adv = - 1 * discrepancy(pred_t1, pred_t2)
        if recipe == 'uda':
            loss_s = loss_s1 + loss_s2
            loss = weight * loss_s + loss_adv
        else:
            loss_s = 0.5 * loss_s1 + 0.5 * loss_s2
            loss_t1 = criterion(pred_t1, label)
            loss_t2 = criterion(pred_t2, label)
            loss_t = 0.5 * loss_t1 + 0.5 * loss_t2
            loss = 0.5 * weight * loss_s + loss_adv + 0.5 * target_loss * loss_t
        loss.backward()
        optimizer_g.step()
        optimizer_c.step()
        optimizer_g.zero_grad()
        optimizer_c.zero_grad()
        feat_node_s = model(data, node_adaptation_s=True)
        feat_node_t = model(data_t, node_adaptation_t=True)
        if recipe == 'uda':
            loss_node_adv = 1 * mmd.mix_rbf_mmd2(feat_node_s, feat_node_t, [0.01, 0.1, 1, 10, 100])
        else:
            loss_node_adv = 1 * mmd.mmd_cal(label, feat_node_s, label_t, feat_node_t, CLASS_MMD)
        loss = loss_node_adv
        loss.backward()
        optimizer_dis.step()
        optimizer_dis.zero_grad()
        losses.append(torch.stack([loss_s.detach(), loss_adv.detach(), loss_node_adv.detach()]))
        shas.append(_sha(model))
    return {'losses': torch.stack(losses).cpu(), 'shas': shas, 'rng': torch.get_rng_state()}


@pytest.mark.parametrize('name', ['Pointnet', 'DGCNN'])
@pytest.mark.parametrize('recipe', ['uda', 'naive_mmd'])
def test_step_is_the_reference_loop_bit_for_bit(recipe, name):
    """UDAStep in its plain form (no graph, composed loss, torch.optim.Adam, separate passes) against the loop of the reference
    written out by hand: B = 4, N = 1024, dropout 0, four steps, one seed -- every loss, sha256(state_dict) after every step and
    the CPU generator's state.  Pins the optimizers' order, the zeroing and the pred_offset carry-over ('naive_mmd' with
    TARGET_LOSS = 1: the target rows scored against the source labels)."""
    want = _literal_loop(name, recipe, 4)
    got = _run(name, steps=4, partial_every=0, recipe=recipe, target_loss=1.0, use_graph=False, fused_loss=False, fused_adam=False,
               pair_domains=False)
    assert torch.isfinite(want['losses']).all()
    assert torch.equal(got['losses'], want['losses']), (got['losses'], want['losses'])
    assert got['shas'] == want['shas'], [i for i, (a, b) in enumerate(zip(got['shas'], want['shas'])) if a != b]
    assert torch.equal(got['rng'], want['rng'])
    net = got['net']
    off = [p for k, p in net.g.named_parameters() if 'pred_offset' in k]
    fresh = [p for k, p in _net(name).g.named_parameters() if 'pred_offset' in k]
    assert off and all(not torch.equal(a.detach(), b.detach()) for a, b in zip(off, fresh))         # optimizer_dis moves them


# ------------------------------------------------------------------------------------------------ 3. the CPU oracle
_ORACLE, _GPU_RUNS = {}, {}


def _oracle_two_steps(dtype=torch.float32, seed=3, lr=1e-3, wd=5e-5):
    """Two steps of recipe 'uda' on Pointnet by the oracle on this machine's CPU (O.net_mda, O.mix_rbf_mmd2, three
    torch.optim.Adam; the FPS starts from the CPU generator at the same seed), computed once per dtype.  Returns the losses, each
    step's phase-2 loss as a STALE run would give it -- the same starts, the weights from before that step's g / c update -- and the
    final parameters."""
    if (dtype, lr) in _ORACLE:
        return _ORACLE[(dtype, lr)]
    from sug_amd.model.Model import Net_MDA
    sd = O.fill_params({k: tuple(v.shape) for k, v in Net_MDA('Pointnet').state_dict().items()}, seed)
    p = O.as_params({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()})
    names = list(p.keys())
    og = torch.optim.Adam([p[k] for k in names if k.startswith('g.') and p[k].requires_grad and 'pred_offset' not in k], lr=lr, weight_decay=wd)
    oc = torch.optim.Adam([p[k] for k in names if k.startswith(('c1.', 'c2.')) and p[k].requires_grad], lr=lr * 2, weight_decay=wd)
    od = torch.optim.Adam([p[k] for k in names if k.startswith(('g.', 'attention')) and p[k].requires_grad], lr=lr, weight_decay=wd)
    data, lab, data_t, lab_t = _batches()[0]
    data, data_t = data.to(dtype), data_t.to(dtype)
    node_loss = lambda q: O.mix_rbf_mmd2(O.net_mda(q, 'Pointnet', data, True, None, node_adaptation_s=True),
                                         O.net_mda(q, 'Pointnet', data_t, True, None, node_adaptation_t=True))
    torch.manual_seed(seed)
    losses, stale = [], []
    for i in range(2):
        ps1, ps2 = O.net_mda(p, 'Pointnet', data, True, None)
        pt1, pt2 = O.net_mda(p, 'Pointnet', data_t, True, None)
        loss_s = F.cross_entropy(ps1, lab) + F.cross_entropy(ps2, lab)
        loss_adv = -torch.mean(torch.abs(F.softmax(pt1, dim=-1) - F.softmax(pt2, dim=-1)))
        (loss_s + loss_adv).backward()
        before = {k: v.detach().clone() for k, v in p.items()}
        og.step(); oc.step()
        og.zero_grad(); oc.zero_grad()
        rng = torch.get_rng_state()
        with torch.no_grad():                               # the stale run: this phase's starts, the weights of before the update
            stale.append(node_loss(before).item())
        torch.set_rng_state(rng)
        loss_node = node_loss(p)
        loss_node.backward()
        od.step()
        od.zero_grad()
        losses.append([loss_s.item(), loss_adv.item(), loss_node.item()])
    _ORACLE[(dtype, lr)] = (losses, stale, {k: v.detach().clone() for k, v in p.items()})
    return _ORACLE[(dtype, lr)]


def _gpu_two_steps(use_graph, seed=3, lr=1e-3):
    """The same two steps by UDAStep with its default options (fused loss, paired domains, sug_amd.optim.Adam), once per form."""
    if (use_graph, lr) not in _GPU_RUNS:
        from sug_amd.uda_step import UDAStep
        net = _net('Pointnet', seed)
        tr = UDAStep(net, recipe='uda', lr=lr, weight_decay=5e-5, use_graph=use_graph)
        data, lab, data_t, lab_t = (t.to(DEV) for t in _batches()[0])
        torch.manual_seed(seed)
        got = [[float(v) for v in tr.step(data, lab, data_t, lab_t)] for _ in range(2)]
        if use_graph:                                       # step 1 planned, step 2 captured and replayed
            assert tr.stats == {'planned': 1, 'captured': 1, 'replayed': 1, 'refused': 0}, (tr.stats, tr.why)
        _GPU_RUNS[(use_graph, lr)] = (got, {k: v.detach().cpu() for k, v in net.state_dict().items()})
    return _GPU_RUNS[(use_graph, lr)]


@pytest.mark.parametrize('use_graph', [False, True])
def test_first_step_matches_the_cpu_oracle_and_would_see_stale_weights(use_graph):
    """B = 4, N = 1024, eager and graph form: the three losses of step 1 within 1e-4 * max(1, |ref|).  Step 1's phase-2 loss is
    computed after the g / c update as well, and the oracle's value for it from the weights of BEFORE the update lies outside that
    bound (measured 2.04899 against 2.04868: 3.1e-4 > 2.05e-4), so this comparison fails on a stale weight copy.  Step 2's phase-2
    loss differs from its stale run too (2.048347 against 2.048174), but by less than the 5e-3 allowed at step 2: there the
    evidence is step 1's.
    Step 2 against the reference's own error: the fp32 oracle is held against the same oracle run in fp64, and the HIP path may
    be at most 3 x as far from the fp64 run + 5e-3 (the project's rule for fp32 errors, tests/test_gpu_source_step.py)."""
    (got, _), (want, stale, _) = _gpu_two_steps(use_graph), _oracle_two_steps()
    want64 = _oracle_two_steps(torch.float64)[0]
    print('losses gpu', got)
    print('losses oracle fp32', want, 'fp64', want64, 'stale phase 2', stale)
    for a, b in zip(got[0], want[0]):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, want)
    assert abs(stale[0] - want[0][2]) > 1e-4 * max(1.0, abs(want[0][2])), (stale, want)
    assert stale[1] != want[1][2]
    for a, b, c in zip(got[1], want[1], want64[1]):
        assert abs(a - c) <= 3.0 * abs(b - c) + 5e-3, (got, want, want64)


# The learning rate of the two comparisons of step 2 below.  Adam's first update moves every weight by the full rate along the
# sign of its gradient, and with these weights (BatchNorm over four rows) the loss is steep: one step takes loss_s from 7.03 to 3.9
# at 1e-3 and still to 6.41 at 1e-6.  An element of the input transform (g.trans_net1.fc3.weight: d loss_s / dw up to 45) whose
# phase-2 gradient is rounding noise -- the reference's fp32 mix_rbf_mmd2 backward adds kernel terms of 1e-6 to a diagonal term of
# 315, the sigma = 0.01 kernel's -- moves the other way and shifts loss_s by 45 * 2 * lr.  The oracle's OWN step-2 loss_s, same
# seed, fp32 with one thread / fp32 with eight threads / fp64:  lr 1e-3: 3.935 / 4.024 / 4.047,  1e-4: 5.593 / 5.760 / 5.142,
# 1e-5: 5.8207 / 5.8194 / 5.4880,  1e-6: 6.40867 / 6.40865 / 6.40709.  1e-6 is the largest power of ten at which the reference
# agrees with itself within a third of the 5e-3 allowed (1.6e-3 against fp64, 3e-5 between thread counts); the update still
# moves loss_s by 0.62, 120 times the bound, so a missing, doubled or misordered update is seen.  (Step 1, and that phase 2 sees
# the updated weights, are checked at 1e-3 above, where one step is well conditioned.)
_LR2 = 1e-6


@pytest.mark.parametrize('use_graph', [False, True])
def test_second_step_losses_match_the_cpu_oracle(use_graph):
    """Step-2 losses within 5e-3 of the fp32 oracle on this machine's CPU, at the learning rate at which the oracle agrees with
    itself (_LR2 above); the first update must have moved loss_s by far more than the bound, or the comparison shows nothing."""
    (got, _), (want, _, _) = _gpu_two_steps(use_graph, lr=_LR2), _oracle_two_steps(lr=_LR2)
    print('step 1: gpu', got[0], 'oracle', want[0])
    print('step 2: gpu', got[1], 'oracle', want[1])
    assert abs(want[1][0] - want[0][0]) > 100 * 5e-3, want
    for a, b in zip(got[0], want[0]):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, want)
    for a, b in zip(got[1], want[1]):
        assert abs(a - b) <= 5e-3, (got, want)


@pytest.mark.parametrize('use_graph', [False, True])
def test_parameter_checksums_after_two_steps_match_the_cpu_oracle(use_graph):
    """The allowance of tests/test_gpu_step.py:95-107 at this run's learning rate (_LR2): Adam's first updates are ~ lr * sign(g),
    an element whose gradient is rounding noise may move the other way -- 4% of the elements, two steps of lr each; running
    statistics absorb such moves."""
    (_, sd), (_, _, p) = _gpu_two_steps(use_graph, lr=_LR2), _oracle_two_steps(lr=_LR2)
    over = []
    for k in p:
        if not p[k].dtype.is_floating_point:
            continue
        v, r = sd[k].double(), p[k].detach().double()
        allow = 0.04 * 2 * 2 * _LR2 * v.numel() + 1e-4 * float(r.abs().sum()) + 1e-6
        if O.is_buffer(k):
            allow = 1e-3 * v.numel() + 1e-3 * float(r.abs().sum())
        d = abs(float(v.sum() - r.sum()))
        if d > allow:
            over.append((k, v.numel(), '%.3g' % d, '%.3g' % allow))
    print('checksums over the allowance (key, elements, deviation, allowance):', over)
    assert not over, over


# ------------------------------------------------------------------------------------------------ 4. graph == eager
@pytest.fixture
def ptran_fp16():
    from sug_amd.model import Ptran_transformer as PT
    keep = PT.GEMM_DTYPE, PT.PROJ_16BIT
    PT.GEMM_DTYPE, PT.PROJ_16BIT = torch.float16, True
    yield
    PT.GEMM_DTYPE, PT.PROJ_16BIT = keep


def _graph_equals_eager(name, recipe):
    kw = dict(recipe=recipe, target_loss=1.0, epoch_at=4)
    e = _run(name, use_graph=False, **kw)
    g = _run(name, use_graph=True, **kw)
    st = g['tr'].stats
    assert st['refused'] == 0 and st['captured'] == 2, (st, g['tr'].why)
    assert st == {'planned': 2, 'captured': 2, 'replayed': 6, 'refused': 0}, st      # steps 1 3 4 6 7 of B = 4, step 5 of B = 3
    assert torch.isfinite(e['losses']).all()
    assert torch.equal(e['losses'], g['losses']), (e['losses'], g['losses'])
    assert e['shas'] == g['shas'], [i for i, (a, b) in enumerate(zip(e['shas'], g['shas'])) if a != b]
    assert torch.equal(e['rng'], g['rng'])
    assert e['tr'].epoch_totals() == g['tr'].epoch_totals()


@pytest.mark.parametrize('name, recipe', [('Pointnet', 'uda'), ('Pointnet2', 'naive_mmd'), ('DGCNN', 'uda'), ('PTran', 'naive_mmd')])
def test_graph_step_equals_eager_step_bit_for_bit(name, recipe):
    """Default options; B = 4 with a partial batch of 3 every third step (a second key), N = 1024, two alternated batches, dropout
    0, eight steps, set_epoch(7, 20) before the fifth (all three rates change; the captured graphs go on): every loss,
    sha256(state_dict) after every step, the CPU generator's final state (the FPS start draws) and the books."""
    _graph_equals_eager(name, recipe)


def test_graph_step_equals_eager_step_ptran_fp16(ptran_fp16):
    """The Point Transformer's fp16 mode: the 16-bit weight copies of phase 2 are made after the g / c update, in both forms."""
    _graph_equals_eager('PTran', 'uda')


# ------------------------------------------------------------------------------------------------ 5. fused + paired
def _one_step(name, recipe, **kw):
    """One step at learning rate 0 with torch.optim.Adam: the losses of both phases, the gradients of both phases as the
    optimizers' first moments (exp_avg = 0.1 * (grad + weight_decay * p) after one step) and the BatchNorm buffers."""
    from sug_amd.uda_step import UDAStep
    net = _net(name)
    tr = UDAStep(net, recipe=recipe, target_loss=1.0, lr=0.0, use_graph=False, fused_adam=False, **kw)
    x, lab, xt, lab_t = (t.to(DEV) for t in _batches()[0])
    torch.manual_seed(5)
    losses = [float(v) for v in tr.step(x, lab, xt, lab_t)]
    names = {id(p): k for k, p in net.named_parameters()}
    grads = {}
    for tag, opt in (('g', tr.optimizer_g), ('c', tr.optimizer_c), ('dis', tr.optimizer_dis)):
        for p, st in opt.state.items():
            grads[tag + ':' + names[id(p)]] = st['exp_avg'].detach().clone() * 10.0
    bufs = {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k}
    return losses, grads, bufs


@pytest.mark.parametrize('name, recipe', [('Pointnet', 'naive_mmd'), ('DGCNN', 'uda')])
def test_fused_loss_and_paired_domains_match_the_composed_separate_form(name, recipe):
    """Tolerances of tests/test_gpu_step.py::test_pair_domains_match_separate_passes (losses 2e-5 relative; gradients rtol 2e-3,
    atol 2e-4 of the largest; BatchNorm buffers rtol 1e-5, atol 1e-6).  Learning rate 0, so that phase 2 of both forms runs on
    the same weights and the comparison is of the arithmetic alone (the update between the phases: sections 2 - 4)."""
    a = _one_step(name, recipe, fused_loss=False, pair_domains=False)
    b = _one_step(name, recipe)
    print(a[0], b[0])
    for x, y in zip(a[0], b[0]):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(x)), (a[0], b[0])
    assert a[1].keys() == b[1].keys() and any(k.startswith('dis:g.') and 'pred_offset' in k for k in a[1])
    gmax = max(float(g.abs().max()) for g in a[1].values())
    for k in a[1]:
        torch.testing.assert_close(b[1][k], a[1][k], rtol=2e-3, atol=2e-4 * gmax)
    for k in a[2]:
        torch.testing.assert_close(b[2][k].float(), a[2][k].float(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 6. books and fallbacks
def _focal():
    from sug_amd.model.model_utils import focal_loss
    c = focal_loss(num_classes=10)
    c.alpha = c.alpha.to(DEV)           # a plain attribute, not a buffer: moved by hand so that its forward copies nothing
    return c


@pytest.mark.parametrize('crit', ['ce', 'focal'])
def test_epoch_totals_are_the_sums_of_loss_times_rows(crit):
    """Six steps in graph form (two keys): the fused kernel keeps the books with nn.CrossEntropyLoss; focal_loss takes the
    composed tail, is captured as well, and keeps them by in-place adds."""
    r = _run('Pointnet', steps=6, hashes=False, recipe='naive_mmd', criterion=None if crit == 'ce' else _focal())
    tr = r['tr']
    assert tr.stats == {'planned': 2, 'captured': 2, 'replayed': 4, 'refused': 0}, (tr.stats, tr.why)      # steps 1 3 4 and 5
    want = [0.0, 0.0, 0.0]
    for ls, rows in zip(r['losses'].tolist(), r['rows']):
        for j in range(3):
            want[j] += ls[j] * rows
    got = tr.epoch_totals()
    assert got[3] == got[4] == float(sum(r['rows']))
    for a, b in zip(got[:3], want):
        assert abs(a - b) <= 4 * np.finfo(np.float64).eps * abs(b), (got, want)
    assert tr.epoch_totals() == (0.0, 0.0, 0.0, 0.0, 0.0)
    x, lab, xt, lab_t = (t.to(DEV) for t in _batches()[0])
    ls = tr.step(x, lab, xt, lab_t)     # the books go on after a reset, in the same captured graph
    assert tr.epoch_totals(reset=False) == (float(ls[0]) * 4, float(ls[1]) * 4, float(ls[2]) * 4, 4.0, 4.0)


def test_kpconv_backbone_runs_eagerly_with_the_reason_recorded():
    from conftest import ROOT
    from sug_amd.model.Model import Net_MDA
    from sug_amd.uda_step import UDAStep
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'kpconv.npz'))
    shapes = {k: tuple(int(s) for s in sh.split(',') if s) for k, sh in zip(z['net_keys'], z['net_shapes'])}
    sd = O.fill_params(shapes, 7)
    for k, v in zip(z['net_kp_keys'], z['net_kp']):
        sd[k] = torch.from_numpy(v)
    net = Net_MDA('KPConv')
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).train()
    x = torch.from_numpy(z['x']).to(DEV)
    xt = x.flip(2).contiguous()
    lab = (torch.arange(x.shape[0], device=DEV) % 10).long()
    tr = UDAStep(net, use_graph=True)
    assert not tr.use_graph and not tr.pair_domains and tr.why is not None and 'KPConv' in tr.why
    got = torch.stack([torch.stack(tr.step(x, lab, xt, lab)) for _ in range(2)]).cpu()
    assert tr.stats == {'planned': 0, 'captured': 0, 'replayed': 0, 'refused': 0}
    assert torch.isfinite(got).all() and got[0, 0] > 0 and got[0, 1] <= 0
    assert tr.epoch_totals()[3:] == (2.0 * x.shape[0], 2.0 * x.shape[0])


def test_per_call_graphs_decline_inside_a_step():
    """With Net_MDA.call_graphs = 'auto' (the product's default; this suite's conftest switches it off) the model(...) calls of
    an eager, unpaired step run inside the step's scope: the per-call graph manager captures nothing, and the step computes
    what it computes with call graphs off."""
    from sug_amd.model.Model import Net_MDA
    kw = dict(steps=3, partial_every=0, use_graph=False, pair_domains=False)
    off = _run('Pointnet', **kw)
    keep, Net_MDA.call_graphs = Net_MDA.call_graphs, 'auto'
    try:
        on = _run('Pointnet', **kw)
    finally:
        Net_MDA.call_graphs = keep
    mgr = on['net'].__dict__.get('_call_graph_mgr')
    assert mgr is None or (not mgr.keys and mgr.stats == {'eager': 0, 'captured': 0, 'replayed': 0, 'refused': 0}), mgr.stats
    assert torch.equal(on['losses'], off['losses']) and on['shas'] == off['shas'] and torch.equal(on['rng'], off['rng'])
