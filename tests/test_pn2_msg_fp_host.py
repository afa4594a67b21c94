"""CPU: multi-scale grouping / feature propagation / TransitionUp -- what can be held without a GPU.

  * the four classes import from sug_amd.model.* and their state_dict keys and shapes are the ones the reference run recorded
    in tests/golden/pn2_msg_fp.npz (so a reference state_dict loads with strict=True);
  * the new entry points are declared in include/sug_amd.h and in sug_amd._lib.SIGNATURES;
  * the torch restatement of tests/pn2_msg_fp_cases.py reproduces the fixture: index lists exactly, fp32 values within 1e-6
    (relative to max(1, |reference|), as tests/test_oracle_golden.py holds the oracle), fp64 values within 1e-9 -- the GPU
    tests use it as the reference at sizes the fixture cannot hold."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import pn2_msg_fp_cases as C

NEW_SYMBOLS = ('sug_ball_query_multi', 'sug_three_nn_direct', 'sug_fp_interp_fwd', 'sug_fp_interp_bwd')
RADII, NSAMPLE = (0.1, 0.2, 0.4), (32, 64, 128)


@pytest.fixture(scope='module')
def G():
    return load_golden('pn2_msg_fp.npz')


def names(v):
    """A name list of the fixture (an empty one loads as an empty numeric tensor)."""
    if isinstance(v, list):
        return v
    assert v.numel() == 0
    return []


def close(a, b, tol, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, '%s: shape %s vs %s' % (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, '%s: max abs err %.3e (scale %.3g, tol %.1e)' % (what, err, scale, tol)


def test_classes_import_with_the_reference_state_dict_layout(G):
    from sug_amd.model.pointnet2_utils import PointNetSetAbstractionMsg, PointNetFeaturePropagation      # noqa: F401
    from sug_amd.model.PTran_utils import PointNetFeaturePropagation as PTranFP                            # noqa: F401
    from sug_amd.model.Ptran_model import TransitionUp                                                     # noqa: F401
    fam = C.hip_family()
    for name, (kind, args, _) in C.CASES.items():
        sd = getattr(fam, kind)(*args).state_dict()
        assert list(sd.keys()) == names(G[name + '_keys']), name
        assert [','.join(map(str, v.shape)) for v in sd.values()] == names(G[name + '_shapes']), name
    sd = C.SegNet(fam).state_dict()
    assert list(sd.keys()) == G['net_keys']
    assert [','.join(map(str, v.shape)) for v in sd.values()] == G['net_shapes']
    # the restatement has the same layout, so one seeded fill serves the reference, the restatement and the HIP classes
    assert list(C.SegNet(C.Restated).state_dict().keys()) == G['net_keys']


def test_new_entry_points_are_declared():
    import ctypes
    from sug_amd import _lib
    for n in NEW_SYMBOLS:
        assert n in _lib.DECLARATIONS and _lib.DECLARATIONS[n][0] is ctypes.c_int, n + ' is not declared in include/sug_amd.h'
        assert n in _lib.SIGNATURES, n + ' is not in _lib.SIGNATURES'
    assert _lib.CONSTANTS['SUG_ABI_VERSION'] == 8


def test_classes_refuse_cpu_tensors():
    fam = C.hip_family()
    args, _ = C.case_inputs('fp_basic')
    with pytest.raises(RuntimeError, match='HIP device'):
        C.build(fam, 'fp_basic')(*args)
    args, _ = C.case_inputs('msg_xyz')
    with pytest.raises(RuntimeError, match='HIP device'):
        C.build(fam, 'msg_xyz')(*args)


def test_restated_operators_reproduce_the_fixture(G):
    from oracle import ref_cpu as O
    rows = C.clouds(C.BQ_SEED, 1024).permute(0, 2, 1).contiguous()
    torch.manual_seed(C.BQ_SEED + 1)
    fps = O.fps_cl(rows, 512)
    assert torch.equal(fps, G['bq_fps'])
    cen = O.gather_cl(rows, fps)
    for i, (r, K) in enumerate(zip(RADII, NSAMPLE)):
        idx = C.ball_lists(r, K, rows, cen)
        if 'bq_idx%d' % i in G:
            assert torch.equal(idx, G['bq_idx%d' % i]), 'ball-query lists, radius %g' % r
        else:
            assert C.list_hash(idx) == G['bq_idx%d_sha256' % i][0], 'ball-query lists, radius %g (hash)' % r
            assert torch.equal(torch.gather(idx, 1, C.subset(512, C.BQ_SEED).unsqueeze(-1).expand(-1, -1, K)), G['bq_idx%d_sub' % i])
    for c in range(4):
        N, S, seed = (int(v) for v in G['nn%d_meta' % c])
        xyz1 = C.clouds(seed, N).permute(0, 2, 1).contiguous()
        xyz2 = O.gather_cl(xyz1, G['nn%d_fps' % c])
        p2 = C.feats(seed, 16, S, 'p2').permute(0, 2, 1).contiguous()
        ids = C.subset(N, seed)
        for form in ('exp', 'dir'):
            pre = 'nn%d_%s_' % (c, form)
            assert torch.equal(G[pre + 'idx32'], G[pre + 'idx64'])          # the generator's precondition
            for dt, tag, tol in ((torch.float32, '32', 1e-6), (torch.float64, '64', 1e-9)):
                _, idx = C.three_nn(xyz1.to(dt), xyz2.to(dt), form == 'dir')
                assert torch.equal(idx, G[pre + 'idx' + tag]), pre + tag
                y = C.interpolate(xyz1.to(dt), xyz2.to(dt), p2.to(dt), form == 'dir').permute(0, 2, 1)
                close(C.take_points(y, ids), G[pre + 'sub' + tag], tol, pre + 'interpolation fp' + tag)
                pr = C.probe(y.shape, 'interp').double()
                close(np.array([y.double().norm().item(), (y.double() * pr).sum().item()]), G[pre + 'stat' + tag], 10 * tol,
                      pre + 'norm / probe fp' + tag)


def _check_run(G, pre, name, res, tag, tol, gtol):
    out = C.case_out(name, res['out']) if name in C.CASES else res['out']
    ids = C.case_ids(name, out.shape[2]) if name in C.CASES else C.subset(out.shape[2], int(G['net_seed']) if 'net_seed' in G else 95)
    if pre + 'out' + tag in G:
        close(out if ids is None else C.take_points(out, ids), G[pre + 'out' + tag], tol, pre + 'output fp' + tag)
    pr = C.probe(out.shape, 'stat').double()
    close(np.array([out.double().norm().item(), (out.double() * pr).sum().item()]), G[pre + 'stat' + tag], 10 * tol, pre + 'stat fp' + tag)
    if pre + 'aux' in G:
        assert torch.equal(res['aux'].float(), G[pre + 'aux']), pre + 'sampled points'
    if 'grad_names' in res:
        assert res['grad_names'] == names(G[pre + 'grad_names']), pre
        gn, gd = np.asarray(G[pre + 'grad_norm' + tag], dtype=np.float64), np.asarray(G[pre + 'grad_dot' + tag], dtype=np.float64)
        floor = gtol * gn.max()
        for k, n, d, a, b in zip(res['grad_names'], res['grad_norm'], res['grad_dot'], gn, gd):
            assert abs(n - a) <= gtol * a + floor, '%s%s: grad norm %.8g vs %.8g' % (pre, k, n, a)
            assert abs(d - b) <= gtol * max(abs(b), a) + floor, '%s%s: grad probe %.8g vs %.8g' % (pre, k, d, b)
    if tag == '32':
        assert res['bn_names'] == names(G[pre + 'bn_names'])
        for k, v, w in zip(res['bn_names'], res['bn_sum'], G[pre + 'bn_sum'].tolist()):
            assert abs(v - w) <= 1e-5 * max(1.0, abs(w)), '%sBN buffer %s: %.8g vs %.8g' % (pre, k, v, w)


@pytest.mark.parametrize('name', [n for n in C.CASES if n != 'fp_s2'])
def test_restated_classes_reproduce_the_fixture(G, name):
    args, gix = C.case_inputs(name)
    seed = C.CASES[name][2]
    for mode in ('train', 'eval'):
        for dt, tag, tol, gtol in ((torch.float32, '32', 1e-6, 1e-4), (torch.float64, '64', 1e-9, 1e-8)):
            net = C.build(C.Restated, name).to(dt).train(mode == 'train')
            _check_run(G, '%s_%s_' % (name, mode), name, C.run(net, args, gix, seed, dtype=dt), tag, tol, gtol)


def test_two_coarse_points_are_an_error(G):
    assert 'fp_s2_error' in G                     # the reference itself fails there
    args, gix = C.case_inputs('fp_s2')
    with pytest.raises(RuntimeError):
        C.build(C.Restated, 'fp_s2')(*args)


def test_restated_network_reproduces_the_fixture(G):
    xyz = C.clouds(95, 1024)
    for mode, runs in (('train', ((torch.float32, '32', 1e-6, 1e-4), (torch.float64, '64', 1e-9, 1e-8))),
                       ('eval', ((torch.float32, '32', 1e-6, 1e-4),))):
        for dt, tag, tol, gtol in runs:
            net = C.SegNet(C.Restated)
            C.load_seeded(net, 95)
            res = C.run(net.to(dt).train(mode == 'train'), [xyz], [], 95, dtype=dt, loss_kind='square')
            _check_run(G, 'net_%s_' % mode, 'net', res, tag, tol, gtol)
            want = float(G['net_%s_loss%s' % (mode, tag)])
            assert abs(res['loss'] - want) <= 10 * tol * max(1.0, abs(want)), (mode, tag, res['loss'], want)
