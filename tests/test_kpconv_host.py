"""CPU: the KPConv backbone's modules construct with the reference's state_dict layout, the kernel-disposition generator
is deterministic and well formed, and the new ops refuse CPU tensors."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden', 'kpconv.npz')


def _layout(sd):
    return list(sd.keys()), [','.join(map(str, v.shape)) for v in sd.values()]


def test_net_mda_kpconv_state_dict_matches_reference():
    from sug_amd.model.Model import Net_MDA
    z = np.load(GOLD)
    keys, shapes = _layout(Net_MDA('KPConv').state_dict())
    assert keys == list(z['net_keys'])
    assert shapes == list(z['net_shapes'])


def test_kpfcls_state_dict_matches_reference():
    from sug_amd.model.KPConv_model import KPFCls
    z = np.load(GOLD)
    keys, shapes = _layout(KPFCls().state_dict())
    assert keys == list(z['cls_keys'])
    assert shapes == list(z['cls_shapes'])


def test_reference_state_dict_loads_strict():
    from sug_amd.model.Model import Net_MDA
    from oracle.ref_cpu import fill_params
    z = np.load(GOLD)
    shapes = {k: tuple(int(s) for s in sh.split(',') if s) for k, sh in zip(z['net_keys'], z['net_shapes'])}
    sd = fill_params(shapes, 7)
    for k, v in zip(z['net_kp_keys'], z['net_kp']):
        sd[k] = torch.from_numpy(v)
    m = Net_MDA('KPConv')
    m.load_state_dict(sd, strict=True)
    assert not m.g.encoder.encoder_blocks[0].KPConv.kernel_points.requires_grad


def test_kernel_disposition_deterministic_centred_bounded():
    from sug_amd.model.KPConv_blocks import load_kernels
    torch.manual_seed(3)
    a = load_kernels(0.05, 15, 3, 'center')
    torch.manual_seed(3)
    b = load_kernels(0.05, 15, 3, 'center')
    assert a.shape == (15, 3) and np.array_equal(a, b)
    assert np.abs(a[0]).max() == 0.0
    r = np.linalg.norm(a, axis=1)
    assert r.max() <= 0.05 * (1 + 1e-5)
    d = np.linalg.norm(a[:, None] - a[None], axis=2) + np.eye(15)
    assert d.min() > 0.01          # spread out, not collapsed
    torch.manual_seed(4)
    assert not np.array_equal(load_kernels(0.05, 15, 3, 'center'), a)      # the rotation is drawn


def test_unsupported_options_raise():
    from sug_amd.model.KPConv_blocks import KPConv, block_decider
    from sug_amd.model.KPConv_model import KPConvConfig
    for kw in ({'deformable': True}, {'aggregation_mode': 'closest'}, {'KP_influence': 'gaussian'}):
        with pytest.raises(NotImplementedError):
            KPConv(15, 3, 4, 4, 0.024, 0.05, **kw)
    with pytest.raises(NotImplementedError):
        block_decider('nearest_upsample', 0.05, 4, 4, 1, KPConvConfig)


def test_sugstep_refuses_kpconv():
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    with pytest.raises(NotImplementedError, match='four-call'):
        SUGStep(Net_MDA('KPConv'))


def test_kpconv_ops_refuse_cpu_tensors():
    from sug_amd import ops
    x = torch.zeros(8, 4)
    p = torch.zeros(8, 3)
    off = torch.tensor([0, 8], dtype=torch.int32)
    nbr = torch.zeros(8, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.kp_grid_subsample(p, off, 1, 8, 0.1)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.radius_neighbors(p, off, p, off, 0.1, 4)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.radius_reverse(nbr, off, off, 8, 8)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.kpconv(x, p, p, nbr, None, torch.zeros(15, 3), torch.zeros(15, 4, 4), 0.02, off)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.seg_instnorm(x, off, act=True)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.seg_max_pool(x, nbr, None)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.seg_mean(x, off)


def test_sample_index_follows_reference_rule():
    from sug_amd.model.KPConv_blocks import sample_index
    idx = sample_index([130, 40], 64)
    assert idx[:64] == list(range(0, 130, 2))[:64]
    assert idx[64:] == [130 + j for j in list(range(40)) + list(range(24))]
