"""CPU: the source-only Point Transformer classifier (sug_amd.model.Ptran_model) builds with the reference's module names
and state_dict layout, accepts the reference's cfg forms, refuses what its kernels cannot run at construction time, and
the fused head's C entry points are bound with the header's signatures."""
import os
import re
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
    from sug_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sug_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    kinds = {'int': 'i32', 'int64_t': 'i64', 'float': 'f32', 'double': 'f64'}
    for name in ('sug_ptcls_head_supported', 'sug_ptcls_head_fwd', 'sug_ptcls_head_bwd'):
        m = re.search(r'\bint\s+' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert m, name
        want = []
        for arg in m.group(1).split(','):
            arg = ' '.join(arg.split())
            want.append('vp' if '*' in arg else kinds[arg.rsplit(' ', 1)[0].replace('const ', '')])
        got = [{_lib._vp: 'vp', _lib._i32: 'i32', _lib._i64: 'i64', _lib._f32: 'f32', _lib._f64: 'f64'}[t]
               for t in _lib.SIGNATURES[name]]
        assert got == want, name


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
