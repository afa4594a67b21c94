"""GPU: the source-only training step (sug_amd.source_step.SourceStep) and its loss kernel (ops.ce = sug_ce_fwd / sug_ce_bwd).

  1. the kernel against torch in fp64 on the CPU (loss, gradient, NaN contract, determinism, the epoch totals);
  2. SourceStep, eager and graph form, against the reference run of tests/golden/pointnet_cls.npz;
  3. graph replay == eager launches, bit for bit, for the four capturable classifiers;
  4. dropout is live in a replay;  5. the epoch's books;  6. KPFCls runs eagerly;  7. the LRU of captured keys."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _case(M, C, seed, ignore_index=-100, ld=None):
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(M, ld or C, generator=g) * 3.0
    z = wide[:, :C]
    y = torch.randint(0, C, (M,), generator=g)
    if M >= 3:
        y[1::7] = ignore_index                              # ignored rows (row 1, 8, 15, ...)
    return wide, z, y


def _ref64(z, y, ignore_index, eps):
    z64 = z.double().clone().requires_grad_()
    loss = F.cross_entropy(z64, y, ignore_index=ignore_index, label_smoothing=eps)
    loss.backward()
    return loss.detach(), z64.grad


def _ours(zg, yg, ignore_index, eps, totals=None):
    from sug_amd import ops
    zg = zg.detach().requires_grad_()
    loss = ops.ce(zg, yg, ignore_index, eps, totals=totals)
    loss.backward()
    return loss.detach(), zg.grad


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('C', [2, 10, 40, 64])
@pytest.mark.parametrize('M', [1, 3, 65, 1024])
def test_ce_against_fp64(M, C, eps):
    """Loss within 1e-4 of max(1, |ref|); gradient error (relative L2 against fp64) <= 3 x that of F.cross_entropy in fp32 on
    the same GPU + 1e-5 (the rule of tests/test_gpu_model.py:409); two runs bit-identical."""
    _, z, y = _case(M, C, 100 * M + C)
    ref, g64 = _ref64(z, y, -100, eps)
    zg, yg = z.contiguous().to(DEV), y.to(DEV)
    loss, grad = _ours(zg, yg, -100, eps)
    loss_b, grad_b = _ours(zg, yg, -100, eps)
    assert torch.equal(loss, loss_b) and torch.equal(grad, grad_b)
    zt = zg.clone().requires_grad_()
    F.cross_entropy(zt, yg, label_smoothing=eps).backward()
    n64 = max(float(g64.norm()), 1e-30)
    e_gpu = float((grad.cpu().double() - g64).norm()) / n64
    e_ref = float((zt.grad.cpu().double() - g64).norm()) / n64
    err = abs(float(loss) - float(ref))
    print('M=%d C=%d eps=%g: loss %.7g ref %.7g (err %.2e), grad err %.2e, torch fp32 %.2e' % (M, C, eps, float(loss), float(ref),
                                                                                          err, e_gpu, e_ref))
    assert err <= 1e-4 * max(1.0, abs(float(ref)))
    assert e_gpu <= 3.0 * e_ref + 1e-5, (e_gpu, e_ref)
    if M >= 3:
        assert float(grad[1].abs().max()) == 0.0            # an ignored row


@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_ce_strided_logits_and_in_range_ignore_index(eps):
    """A column slice of a wider tensor (ld = 48 > C = 40), ignore_index = 7 (a class of its own, as torch allows)."""
    wide, z, y = _case(65, 40, 5, ignore_index=7, ld=48)
    ref, g64 = _ref64(z, y, 7, eps)
    zs = wide.to(DEV)[:, :40]
    assert zs.stride(0) == 48
    loss, grad = _ours(zs, y.to(DEV), 7, eps)
    assert abs(float(loss) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref)))
    zt = zs.detach().clone().requires_grad_()
    F.cross_entropy(zt, y.to(DEV), ignore_index=7, label_smoothing=eps).backward()
    n64 = float(g64.norm())
    e_gpu, e_ref = float((grad.cpu().double() - g64).norm()) / n64, float((zt.grad.cpu().double() - g64).norm()) / n64
    assert e_gpu <= 3.0 * e_ref + 1e-5, (e_gpu, e_ref)
    assert grad.shape == (65, 40) and grad.is_contiguous()


def test_ce_all_ignored_and_out_of_range_labels():
    _, z, y = _case(5, 10, 9)
    zg = z.to(DEV)
    ignored = torch.full((5,), -100, dtype=torch.long)
    assert torch.isnan(F.cross_entropy(z.double(), ignored))            # what torch returns
    loss, grad = _ours(zg, ignored.to(DEV), -100, 0.0)
    assert torch.isnan(loss) and float(grad.abs().max()) == 0.0
    for bad in (10, -1):                                                # torch raises; the kernel poisons the result
        yb = y.clone()
        yb[3] = bad
        loss, grad = _ours(zg, yb.to(DEV), -100, 0.1)
        assert torch.isnan(loss)
        assert torch.isnan(grad[3]).all() and not torch.isnan(grad[[0, 2, 4]]).any()


def test_ce_totals_accumulate_in_the_same_launch():
    totals = torch.zeros(2, dtype=torch.float64, device=DEV)
    want, rows = 0.0, 0
    for M in (3, 65, 1024):
        _, z, y = _case(M, 10, M)
        loss, _ = _ours(z.to(DEV), y.to(DEV), -100, 0.0, totals=totals)
        want += float(loss) * M                                         # loss_total += loss_s.item() * data.size(0)
        rows += M
    got = totals.tolist()
    assert got[1] == float(rows)
    assert abs(got[0] - want) <= 4 * np.finfo(np.float64).eps * abs(want), (got[0], want)


# ------------------------------------------------------------------------------------------------ models and runs
def _net(name, seed=3, dropout=0.0):
    from sug_amd.model import model_pointnet as MP
    from sug_amd.model.Ptran_model import PointTransformerCls
    net = PointTransformerCls() if name == 'PointTransformerCls' else getattr(MP, name)()
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
    if dropout is not None:
        for m in net.modules():
            if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)):
                m.p = dropout
    return net.to(DEV).train()


_BATCHES = {}


def _batches(B=4, N=1024):
    """Two fixed batches (clouds, labels), made once and never written to."""
    if (B, N) not in _BATCHES:
        g = torch.Generator().manual_seed(17)
        _BATCHES[(B, N)] = [(O.synth_clouds(B, N, g).to(DEV), torch.randint(0, 10, (B,), generator=g).to(DEV)) for _ in range(2)]
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


def _run(name, use_graph, steps=8, sched=None, max_graphs=4, criterion=None, hashes=True, **kw):
    from sug_amd.source_step import SourceStep
    net = _net(name)
    tr = SourceStep(net, use_graph=use_graph, max_graphs=max_graphs, criterion=criterion, **kw)
    torch.manual_seed(11)
    losses, shas = [], []
    for bi, rows in (sched or _schedule(steps)):
        x, lab = _batches()[bi]
        losses.append(tr.step(x[:rows], lab[:rows]))
        if hashes:
            shas.append(_sha(net))
    return {'losses': torch.stack(losses).cpu(), 'shas': shas, 'rng': torch.get_rng_state(), 'tr': tr, 'net': net,
            'rows': [r for _, r in (sched or _schedule(steps))]}


# ------------------------------------------------------------------------------------------------ 2. the reference run
@pytest.mark.parametrize('use_graph', [False, True])
def test_source_step_reproduces_the_reference_run(use_graph):
    """tests/golden/pointnet_cls.npz (B = 8, N = 1024; fill_params at the fixture's seed, dropout 0, lr 1e-3, weight decay
    5e-5): loss, post-step parameters and the second-forward loss within the tolerances of
    tests/test_gpu_model.py::test_pointnet_cls_config1_source_only_train_step.
    Graph form: the readings are taken after the same ONE update, made by a REPLAY.  The key is planned and captured at
    learning rate 0 (set_epoch(50, 50): the parameters do not move; on a fixed batch every step sees the same gradient g, and
    Adam's bias-corrected moments of a constant gradient are g and g^2 at every step count, so the first update at the restored
    rate is the reference's lr * g / (|g| + eps) up to rounding); set_epoch(0, 50) then puts 1e-3 back on the device and the
    same captured graph makes the update."""
    from sug_amd.source_step import SourceStep
    from sug_amd.model.model_pointnet import Pointnet_cls
    G = load_golden('pointnet_cls.npz')
    net = Pointnet_cls()
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, G['seed']))
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    net = net.to(DEV).train()
    p0 = {k: v.detach().clone() for k, v in net.named_parameters()}
    x, lab = G['x'].to(DEV), G['label'].to(DEV)
    lr = 1e-3
    tr = SourceStep(net, lr=lr, weight_decay=5e-5, use_graph=use_graph)
    if use_graph:
        assert tr.set_epoch(50, 50) == 0.0
        tr.step(x, lab)
        tr.step(x, lab)
        assert all(torch.equal(v.detach(), p0[k]) for k, v in net.named_parameters())
        assert tr.set_epoch(0, 50) == lr
    loss = tr.step(x, lab)
    if use_graph:
        assert tr.stats == {'planned': 1, 'captured': 1, 'replayed': 2, 'refused': 0}, (tr.stats, tr.why)
    print('loss %.7g (reference %.7g)' % (float(loss), float(G['loss'])))
    assert abs(float(loss) - float(G['loss'])) <= 1e-4 * max(1.0, abs(float(G['loss'])))
    post = dict(net.named_parameters())
    for k, want_sum, want_dn in zip(G['param_names'], G['param_sum'].tolist(), G['param_delta_norm'].tolist()):
        n = post[k].numel()
        dn = float((post[k].detach() - p0[k]).double().norm())
        assert abs(dn - want_dn) <= 2e-2 * max(want_dn, lr), (k, dn, want_dn)
        got_sum = float(post[k].detach().double().sum())
        assert abs(got_sum - want_sum) <= 2 * lr * max(4.0, 0.01 * n) + 1e-5 * abs(want_sum), (k, got_sum, want_sum, n)
    with torch.no_grad():
        loss2 = F.cross_entropy(net(x), lab)
    assert abs(float(loss2) - float(G['loss2'])) <= 2e-3 * max(1.0, abs(float(G['loss2']))), (float(loss2), float(G['loss2']))
    assert float(loss2) < float(G['loss'])


# ------------------------------------------------------------------------------------------------ 3. graph == eager
@pytest.mark.parametrize('name', ['Pointnet_cls', 'DGCNN', 'Pointnet2_cls', 'PointTransformerCls'])
def test_graph_step_equals_eager_step_bit_for_bit(name):
    """B = 4 with a partial batch of 3 every third step (a second key), N = 1024, two alternated batches, dropout 0, eight
    steps: every loss, sha256(state_dict) after every step and the CPU generator's final state (the FPS start draws)."""
    e = _run(name, False)
    g = _run(name, True)
    st = g['tr'].stats
    assert st['refused'] == 0 and st['captured'] == 2, (st, g['tr'].why)
    assert st == {'planned': 2, 'captured': 2, 'replayed': 6, 'refused': 0}, st      # steps 1 3 4 6 7 of B = 4, step 5 of B = 3
    assert torch.isfinite(e['losses']).all()
    assert torch.equal(e['losses'], g['losses']), (e['losses'], g['losses'])
    assert e['shas'] == g['shas'], [i for i, (a, b) in enumerate(zip(e['shas'], g['shas'])) if a != b]
    assert torch.equal(e['rng'], g['rng'])
    if name == 'DGCNN':                 # constructed and unused, as in the reference: no gradient, skipped by Adam
        assert all(p.grad is None for p in g['net'].input_transform_net.parameters())
        fresh = _net(name).input_transform_net.state_dict()
        assert all(torch.equal(v, fresh[k]) for k, v in g['net'].input_transform_net.state_dict().items()
                   if not k.endswith('num_batches_tracked'))


def test_torch_adam_form_is_captured_too():
    """fused_adam=False: torch.optim.Adam (capturable, fused under a graph).  Its eager twin is torch's default Adam, another
    kernel, so the losses are held to the reference-run tolerance of the second-forward loss (2e-3), not bit for bit."""
    e = _run('Pointnet_cls', False, steps=4, fused_adam=False, hashes=False)
    g = _run('Pointnet_cls', True, steps=4, fused_adam=False, hashes=False)
    assert isinstance(g['tr'].optimizer, torch.optim.Adam) and not hasattr(g['tr'].optimizer, 'graph_key')
    assert g['tr'].stats == {'planned': 2, 'captured': 1, 'replayed': 2, 'refused': 0}, (g['tr'].stats, g['tr'].why)
    assert torch.isfinite(g['losses']).all()
    assert float((e['losses'] - g['losses']).abs().max()) <= 2e-3 * max(1.0, float(e['losses'].abs().max())), (e['losses'], g['losses'])


# ------------------------------------------------------------------------------------------------ 4. dropout
def test_dropout_is_live_in_a_replay():
    """Pointnet_cls with its own Dropout2d(0.7), lr = 0 and weight decay = 0, the same batch every step: the loss changes from
    replay to replay only through the dropout masks; two whole runs from one seed draw the same masks."""
    from sug_amd.source_step import SourceStep
    x, lab = _batches(16)[0]            # Dropout2d on [B, 512] rows drops whole rows: 16 of them, so that two masks differ
    runs = []
    for _ in range(2):
        net = _net('Pointnet_cls', dropout=None)
        tr = SourceStep(net, lr=0.0, weight_decay=0.0, use_graph=True)
        torch.manual_seed(3)
        runs.append(torch.stack([tr.step(x, lab) for _ in range(5)]).cpu())
        assert tr.stats == {'planned': 1, 'captured': 1, 'replayed': 4, 'refused': 0}, (tr.stats, tr.why)
    a = runs[0]
    assert all(float(a[i]) != float(a[i + 1]) for i in range(1, 4)), a      # steps 1 .. 4 are replays
    assert torch.equal(runs[0], runs[1]), runs


# ------------------------------------------------------------------------------------------------ 5. books
def _focal():
    from sug_amd.model.model_utils import focal_loss
    c = focal_loss(num_classes=10)
    c.alpha = c.alpha.to(DEV)           # a plain attribute, not a buffer: moved by hand so that its forward copies nothing
    return c


@pytest.mark.parametrize('crit', ['ce', 'focal'])
def test_epoch_totals_are_the_sum_of_loss_times_rows(crit):
    r = _run('Pointnet_cls', True, steps=6, criterion=None if crit == 'ce' else _focal(), hashes=False)
    tr = r['tr']
    assert tr.stats['captured'] == 2 and tr.stats['refused'] == 0, (tr.stats, tr.why)
    want = 0.0
    for l, rows in zip(r['losses'].tolist(), r['rows']):
        want += l * rows
    loss_total, data_total = tr.epoch_totals()
    assert data_total == float(sum(r['rows']))
    assert abs(loss_total - want) <= 4 * np.finfo(np.float64).eps * abs(want), (loss_total, want)
    assert tr.epoch_totals() == (0.0, 0.0)
    x, lab = _batches()[0]
    l = tr.step(x, lab)                 # the books go on after a reset, in the same captured graph
    assert tr.epoch_totals(reset=False) == (float(l) * 4, 4.0)


# ------------------------------------------------------------------------------------------------ 6. KPFCls
def _kpfcls():
    import os
    from conftest import ROOT
    from sug_amd.model.KPConv_model import KPFCls
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'kpconv.npz'))
    shapes = {k: tuple(int(s) for s in sh.split(',') if s) for k, sh in zip(z['cls_keys'], z['cls_shapes'])}
    sd = O.fill_params(shapes, 7)
    for k, v in zip(z['cls_kp_keys'], z['cls_kp']):
        sd[k] = torch.from_numpy(v)
    m = KPFCls()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(), torch.from_numpy(z['x']).to(DEV)


def test_kpfcls_runs_eagerly_and_equals_the_hand_written_loop():
    """KPFCls at the shape of tests/test_gpu_kpconv.py: never captured, the reason recorded, and every loss equal, bit for bit,
    to the loop of train_source.py:113-131 written out by hand with the same ops (ops.ce as the criterion, the regulariser,
    sug_amd.optim.Adam); against that loop with nn.CrossEntropyLoss the loss holds the project's 1e-4."""
    from sug_amd import ops
    from sug_amd.model.KPConv_model import p2p_fitting_regularizer
    from sug_amd.optim import Adam
    from sug_amd.source_step import SourceStep
    net, x = _kpfcls()
    lab = (torch.arange(x.shape[0], device=DEV) % 10).long()
    tr = SourceStep(net, use_graph=True)
    got = torch.stack([tr.step(x, lab) for _ in range(3)]).cpu()
    assert tr.stats == {'planned': 0, 'captured': 0, 'replayed': 0, 'refused': 0}
    assert tr.why is not None and 'KPFCls' in tr.why
    hand = {}
    for form in ('ops.ce', 'nn'):
        net, x = _kpfcls()
        opt = Adam(net.parameters(), lr=1e-3, weight_decay=5e-5, graph_capturable=True)
        crit = torch.nn.CrossEntropyLoss()
        ls = []
        for _ in range(3):
            out = net(x)
            loss = ops.ce(out, lab) if form == 'ops.ce' else crit(out, lab)
            loss = loss + p2p_fitting_regularizer(net.encoder.encoder_blocks, deform_fitting_power=net.deform_fitting_power)
            loss.backward()
            opt.step()
            opt.zero_grad()
            ls.append(loss.detach())
        hand[form] = torch.stack(ls).cpu()
    assert torch.equal(got, hand['ops.ce']), (got, hand['ops.ce'])
    assert float((got - hand['nn']).abs().max()) <= 1e-4 * max(1.0, float(hand['nn'].abs().max())), (got, hand['nn'])


# ------------------------------------------------------------------------------------------------ 7. LRU
def test_one_graph_slot_with_two_alternating_batch_sizes_stays_correct():
    sched = [(i % 2, 4 if i % 2 == 0 else 3) for i in range(6)]
    e = _run('Pointnet_cls', False, sched=sched)
    g = _run('Pointnet_cls', True, sched=sched, max_graphs=1)
    assert torch.equal(e['losses'], g['losses']) and e['shas'] == g['shas']
    assert g['tr'].stats['refused'] == 0 and len(g['tr']._graphs) == 1
    # and a key that gets its two steps in a row is captured and replayed in the one slot
    sched = [(0, 4), (1, 4), (0, 4), (1, 3), (0, 3), (1, 3)]
    e = _run('Pointnet_cls', False, sched=sched)
    g = _run('Pointnet_cls', True, sched=sched, max_graphs=1)
    assert torch.equal(e['losses'], g['losses']) and e['shas'] == g['shas']
    assert g['tr'].stats == {'planned': 2, 'captured': 2, 'replayed': 4, 'refused': 0}, g['tr'].stats
