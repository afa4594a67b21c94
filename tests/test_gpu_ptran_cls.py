"""GPU: the source-only Point Transformer classifier (sug_amd.model.Ptran_model.PointTransformerCls).

  * the fused head (ops.ptcls_head, sug_ptcls_head_*) against an fp64 torch restatement, forward and every gradient,
    bit-identical across two runs; outside its range the composed library head takes over, also against fp64;
  * the full model against the reference run of tests/golden/ptran_cls.npz (B = 2, N = 1024 and 2048, the CPU-generator
    FPS draws): logits and CE loss within 1e-4, gradients against the reference's fp32 ones and at least as close to the
    fp64 run as those, BatchNorm buffers; one train_source.py step with torch.optim.Adam and sug_amd.optim.Adam; eval-mode
    logits after it; the fp16 projection mode within the Point Transformer's 16-bit bound;
  * eval_worker with source_flag and the graph-replayed eval forward (tests/ptran_cls_eval_cases.py, in a child process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

SEEDS = {1024: 61, 2048: 62}
LR, WD = 5e-4, 1e-4


def probe(shape, tag):
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()) % (2 ** 31))
    return torch.randn(shape, generator=g)


def close(a, b, tol, what):
    a, b = a.detach().cpu().float(), torch.as_tensor(b).float()
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, '%s: max abs err %.3e (scale %.3g, tol %.1e)' % (what, err, scale, tol)
    return err


# ------------------------------------------------------------------------------------------------ the head op
def _fc2(nc, seed):
    torch.manual_seed(seed)
    fc2 = torch.nn.Sequential(torch.nn.Linear(512, 256), torch.nn.ReLU(), torch.nn.Linear(256, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, nc))
    with torch.no_grad():
        for lin in (fc2[0], fc2[2], fc2[4]):
            lin.bias.normal_(0, 0.2)          # both signs of every pre-activation reach the ReLUs
    return fc2.cuda()


def _head_run(fc2, points, gprobe):
    from sug_amd.model.Ptran_model import classify
    for p in fc2.parameters():
        p.grad = None
    pts = points.clone().requires_grad_(True)
    y = classify(fc2, pts)
    (y * gprobe).sum().backward()
    return [y.detach(), pts.grad] + [p.grad.clone() for p in fc2.parameters()]


def _head_fp64(fc2, points, gprobe):
    ps = [p.detach().double().requires_grad_(True) for p in fc2.parameters()]
    pts = points.double().requires_grad_(True)
    h = torch.relu(torch.nn.functional.linear(pts.mean(1), ps[0], ps[1]))
    h = torch.relu(torch.nn.functional.linear(h, ps[2], ps[3]))
    y = torch.nn.functional.linear(h, ps[4], ps[5])
    g = torch.autograd.grad((y * gprobe.double()).sum(), [pts] + ps)
    return [y.detach()] + list(g)


@pytest.mark.parametrize('B,P,nc', [(32, 4, 10), (1, 4, 2), (2, 4, 10), (17, 3, 40), (128, 4, 64), (33, 1, 7),
                                    (129, 4, 10), (8, 4, 65), (8, 4, 1)])
def test_head_against_fp64(B, P, nc):
    from sug_amd import ops
    fc2 = _fc2(nc, B * 100 + nc)
    g = torch.Generator().manual_seed(B + P + nc)
    points = torch.randn(B, P, 512, generator=g).cuda()
    gprobe = torch.randn(B, nc, generator=g).cuda()
    fused = B <= 128 and 2 <= nc <= 64
    assert ops.ptcls_head_supported(points, fc2) == fused
    got = _head_run(fc2, points, gprobe)
    want = _head_fp64(fc2, points, gprobe)
    names = ['logits', 'dpoints', 'dW1', 'db1', 'dW2', 'db2', 'dW3', 'db3']
    for a, b, nm in zip(got, want, names):
        assert a.dtype == torch.float32 and a.shape == b.shape, nm
        err = float((a.double() - b).norm() / b.norm().clamp_min(1e-30))
        assert err < 1e-5, '%s: relative L2 error %.2e against fp64' % (nm, err)
    if fused:
        again = _head_run(fc2, points, gprobe)
        for a, b, nm in zip(got, again, names):
            assert torch.equal(a, b), nm + ' differs between two runs'


def test_head_knob_selects_the_composed_path():
    from sug_amd import ops
    fc2 = _fc2(10, 3)
    points = torch.randn(4, 4, 512).cuda()
    keep = ops.PTCLS_HEAD_FUSED
    try:
        ops.PTCLS_HEAD_FUSED = False
        assert not ops.ptcls_head_supported(points, fc2)
    finally:
        ops.PTCLS_HEAD_FUSED = keep
    assert ops.ptcls_head_supported(points, fc2)


# ------------------------------------------------------------------------------------------------ the full model
def _net(seed):
    from sug_amd.model.Ptran_model import PointTransformerCls
    net = PointTransformerCls()
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
    return net.cuda().train()


def _golden(N):
    G = load_golden('ptran_cls.npz')
    pre = 'n%d_' % N
    return {k[len(pre):]: v for k, v in G.items() if k.startswith(pre)} | {'keys': G['keys']}


def _forward_backward(net, G):
    seed = int(G['seed'])
    x, lab = G['x'].cuda(), G['label'].cuda()
    torch.manual_seed(seed + 1)
    y = net(x)
    loss = torch.nn.functional.cross_entropy(y, lab)
    net.zero_grad()
    loss.backward()
    return y, loss


def _check_forward_backward(net, G, y, loss):
    close(y, G['y'], 1e-4, 'logits')
    assert abs(loss.item() - float(G['loss'])) <= 1e-4 * max(1.0, abs(float(G['loss']))), (loss.item(), float(G['loss']))
    got = dict(net.named_parameters())
    names = list(G['grad_names'])
    assert sorted(names) == sorted(k for k, p in got.items() if p.grad is not None)
    norm = np.array([got[k].grad.double().norm().item() for k in names])
    dot = np.array([(got[k].grad.cpu().double() * probe(got[k].shape, 'g' + k).double()).sum().item() for k in names])
    gn32, gd32, gn64, gd64 = (np.asarray(G[k], dtype=np.float64) for k in ('grad_norm', 'grad_dot', 'grad_norm64', 'grad_dot64'))
    # against the reference's fp32 run, as tests/test_gpu_model.py holds the PTran encoder (norms 2e-2, probe dots 5e-2)
    floor = 1e-4 * gn32.max()
    for k, n, d, a, b in zip(names, norm, dot, gn32, gd32):
        assert abs(n - a) <= 2e-2 * a + floor, '%s: grad norm %.6g vs %.6g' % (k, n, a)
        assert abs(d - b) <= 5e-2 * max(abs(b), a) + floor, '%s: grad probe %.6g vs %.6g' % (k, d, b)
    # against the fp64 run: at least as accurate as the reference's fp32 arithmetic
    for what, ours, ref32, ref64 in (('norm', norm, gn32, gn64), ('probe', dot, gd32, gd64)):
        e_ours, e_32 = np.linalg.norm(ours - ref64), np.linalg.norm(ref32 - ref64)
        print('gradient %s error against fp64: HIP %.3e, reference fp32 %.3e (|fp64| %.3e)'
              % (what, e_ours, e_32, np.linalg.norm(ref64)))
        assert e_ours <= 2 * e_32 + 1e-5 * np.linalg.norm(ref64), (what, e_ours, e_32)
    sd = net.state_dict()
    for k, v in zip(G['bn_names'], G['bn_sum'].tolist()):
        got_sum = sd[k].double().sum().item()
        assert abs(got_sum - v) <= 1e-4 * max(1.0, abs(v)), 'BN buffer %s: %.8g vs %.8g' % (k, got_sum, v)


@pytest.mark.parametrize('N', [1024, 2048])
def test_model_against_reference(N):
    G = _golden(N)
    net = _net(int(G['seed']))
    y, loss = _forward_backward(net, G)
    _check_forward_backward(net, G, y, loss)


@pytest.mark.parametrize('N', [1024, 2048])
def test_source_only_train_step(N):
    """train_source.py:94, :113-131 with Model PTran: forward, CE, backward, ONE Adam update (lr 5e-4, weight decay 1e-4),
    then the loss of a second forward, and eval-mode logits after the step -- with torch.optim.Adam and sug_amd.optim.Adam,
    held to the tolerances of tests/test_gpu_model.py::test_pointnet_cls_config1_source_only_train_step."""
    G = _golden(N)
    seed = int(G['seed'])
    for own_adam in (False, True):
        net = _net(seed)
        p0 = {k: v.detach().clone() for k, v in net.named_parameters()}
        if own_adam:
            from sug_amd.optim import Adam
            opt = Adam(net.parameters(), lr=LR, weight_decay=WD)
        else:
            opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=WD)
        y, loss = _forward_backward(net, G)
        _check_forward_backward(net, G, y, loss)
        opt.step()
        opt.zero_grad()
        post = dict(net.named_parameters())
        for k, want_sum, want_dn in zip(G['param_names'], G['param_sum'].tolist(), G['param_delta_norm'].tolist()):
            n = post[k].numel()
            dn = float((post[k].detach() - p0[k]).double().norm())
            assert abs(dn - want_dn) <= 2e-2 * max(want_dn, LR), (own_adam, k, dn, want_dn)
            got_sum = float(post[k].detach().double().sum())
            assert abs(got_sum - want_sum) <= 2 * LR * max(4.0, 0.01 * n) + 1e-5 * abs(want_sum), (own_adam, k, got_sum, want_sum, n)
        x, lab = G['x'].cuda(), G['label'].cuda()
        torch.manual_seed(seed + 2)
        with torch.no_grad():
            loss2 = torch.nn.functional.cross_entropy(net(x), lab)
        want2 = float(G['loss2'])
        assert abs(float(loss2) - want2) <= 2e-3 * max(1.0, abs(want2)), (own_adam, float(loss2), want2)
        net.eval()
        torch.manual_seed(seed + 3)
        with torch.no_grad():
            y_eval = net(x)
        close(y_eval, G['y_eval'], 2e-3, 'eval-mode logits after the step')


def test_fp16_projection_mode():
    """bench.py --fp16's mode (Ptran_transformer.GEMM_DTYPE = fp16, PROJ_16BIT): logits within the 1e-2 bound
    tests/test_gpu_model.py::test_ptran_reduced_precision_mode_deviation sets for the encoder; gradients flow."""
    from sug_amd.model import Ptran_transformer as PT
    G = _golden(1024)
    seed = int(G['seed'])
    net = _net(seed)
    x = G['x'].cuda()
    with torch.no_grad():
        torch.manual_seed(seed + 1)
        ref = net(x)
    keep = PT.GEMM_DTYPE, PT.PROJ_16BIT
    try:
        PT.GEMM_DTYPE, PT.PROJ_16BIT = torch.float16, True
        torch.manual_seed(seed + 1)
        with torch.no_grad():
            got = net(x)
        torch.manual_seed(seed + 1)
        net(x).square().mean().backward()
    finally:
        PT.GEMM_DTYPE, PT.PROJ_16BIT = keep
    close(got, ref.cpu(), 1e-2, 'fp16 projection mode logits')
    g = net.backbone.transformers[0].fc_gamma[0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert net.fc2[0].weight.grad is not None and bool(torch.isfinite(net.fc2[0].weight.grad).all())


# ------------------------------------------------------------------------------------------------ evaluation
@pytest.fixture(scope='module')
def eval_cases(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('ptran_cls_eval') / 'results.json')
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(ROOT, 'tests', 'ptran_cls_eval_cases.py'), out]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    res = json.load(open(out)) if os.path.exists(out) else {}
    return res, r


def _check_case(eval_cases, name):
    res, r = eval_cases
    if name not in res:
        pytest.fail('the case process ended (exit %d) before case %s:\n%s' % (r.returncode, name, r.stderr.decode()[-3000:]))
    assert res[name] is None, res[name]


def test_graph_replay_equals_eager_call(eval_cases):
    """EvalRunner on PointTransformerCls: eager, captured and replayed calls equal the eager eval forward bit for bit."""
    _check_case(eval_cases, 'graph_replay_equals_eager_call')


def test_eval_worker_source_flag(eval_cases):
    """eval_worker(source_flag) over two epochs: metrics equal the restated reference loop, every batch of epoch 2 replayed."""
    _check_case(eval_cases, 'eval_worker_source_flag_two_epochs')
