"""CPU: the source-only Point Transformer classifier (sug_amd.model.Ptran_model) builds with the reference's module names
and state_dict layout, accepts the reference's cfg forms, refuses what its kernels cannot run at construction time, and
the fused head's C entry points are bound with the header's signatures."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden', 'ptran_cls.npz')


def _cfg(**over):
    model = {'nneighbor': 16, 'nblocks': 4, 'transformer_dim': 512}
    model.update({k: over.pop(k) for k in list(over) if k in model})
    d = {'num_point': 1024, 'num_class': 10, 'input_dim': 3, 'model': model}
    d.update(over)
    return d


def _ns(d):
    return types.SimpleNamespace(**{k: _ns(v) if isinstance(v, dict) else v for k, v in d.items()})


def test_module_exports_the_three_classes():
    from sug_amd.model import Ptran_model as PM
    for name in ('TransitionDown', 'Backbone', 'PointTransformerCls'):
        assert isinstance(getattr(PM, name), type) and issubclass(getattr(PM, name), torch.nn.Module)
        assert name in PM.__all__


def test_state_dict_layout_matches_reference():
    from sug_amd.model.Ptran_model import PointTransformerCls
    z = np.load(GOLD)
    sd = PointTransformerCls().state_dict()
    assert list(sd.keys()) == list(z['keys'])
    assert [','.join(map(str, v.shape)) for v in sd.values()] == list(z['shapes'])


def test_reference_state_dict_loads_strict():
    from sug_amd.model.Ptran_model import PointTransformerCls
    from oracle.ref_cpu import fill_params
    z = np.load(GOLD)
    shapes = {k: tuple(int(s) for s in sh.split(',') if s) for k, sh in zip(z['keys'], z['shapes'])}
    sd = fill_params(shapes, 5)
    m = PointTransformerCls()
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.fc2[4].bias, sd['fc2.4.bias'])
    assert torch.equal(m.backbone.transition_downs[3].sa.mlp_convs[1].weight, sd['backbone.transition_downs.3.sa.mlp_convs.1.weight'])


@pytest.mark.parametrize('form', ['none', 'attr', 'dict'])
def test_cfg_forms(form):
    from sug_amd.model.Ptran_model import PointTransformerCls, Backbone
    cfg = {'none': None, 'attr': _ns(_cfg(num_class=40)), 'dict': _cfg(num_class=40)}[form]
    m = PointTransformerCls(cfg)
    assert m.fc2[4].out_features == (10 if form == 'none' else 40)
    assert m.fc2[0].in_features == 512 and m.nblocks == 4
    assert [td.sa.npoint for td in m.backbone.transition_downs] == [256, 64, 16, 4]
    assert m.backbone.transformer1.k == 16 and m.backbone.transformer1.fc1.out_features == 512
    assert isinstance(Backbone(cfg), Backbone)


@pytest.mark.parametrize('field,value', [('input_dim', 6), ('nneighbor', 8), ('nblocks', 3), ('transformer_dim', 256)])
def test_unsupported_cfg_raises_naming_the_field(field, value):
    from sug_amd.model.Ptran_model import PointTransformerCls, Backbone
    for cfg in (_cfg(**{field: value}), _ns(_cfg(**{field: value}))):
        for cls in (PointTransformerCls, Backbone):
            with pytest.raises(NotImplementedError, match=field):
                cls(cfg)


def test_cpu_input_raises_gpu_only_message():
    from sug_amd.model.Ptran_model import PointTransformerCls
    with pytest.raises(RuntimeError, match='HIP device'):
        PointTransformerCls()(torch.zeros(2, 3, 1024, 1))


def test_ptcls_head_ctypes_signatures_match_header():
    """The binding is derived from the header; these lists are written by hand from the three prototypes."""
    from sug_amd._lib import SIGNATURES, _vp, _i32
    assert SIGNATURES['sug_ptcls_head_supported'] == [_i32] * 6                                          # B P K N1 N2 NC
    assert SIGNATURES['sug_ptcls_head_fwd'] == (
        [_vp, _i32, _i32, _i32] + [_vp, _vp, _i32] * 3          # points B P K, then (W, b, N) of the three layers
        + [_vp] * 5)                                            # mean h1 h2 logits stream
    assert SIGNATURES['sug_ptcls_head_bwd'] == (
        [_vp] * 4 + [_i32, _i32, _i32] + [_vp, _i32] * 3        # dlogits mean h1 h2, B P K, then (W, N) of the three layers
        + [_vp] * 3 + [_vp] * 6 + [_vp])                        # dz1 dz2 dpoints, dW1 db1 dW2 db2 dW3 db3, stream


def test_ptcls_head_supported_range():
    from sug_amd import _lib
    L = _lib.lib()
    assert L.sug_ptcls_head_supported(32, 4, 512, 256, 64, 10) == 1
    assert L.sug_ptcls_head_supported(128, 4, 512, 256, 64, 64) == 1
    assert L.sug_ptcls_head_supported(1, 4, 512, 256, 64, 2) == 1
    assert L.sug_ptcls_head_supported(129, 4, 512, 256, 64, 10) == 0
    assert L.sug_ptcls_head_supported(32, 4, 512, 256, 64, 65) == 0
    assert L.sug_ptcls_head_supported(32, 4, 512, 256, 64, 1) == 0
    # argument validation happens on the host before any launch: safe without a GPU
    assert L.sug_ptcls_head_fwd(None, 200, 4, 512, None, None, 256, None, None, 64, None, None, 10,
                                None, None, None, None, None) == -1
    assert b'unsupported' in L.sug_last_error()
