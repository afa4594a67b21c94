"""CPU: the host side of the KPConv capacity layout -- the capacity formula, the validation of set_level_caps, the
graph_capturable flag following the caps, the refusals that stay, and the declared / exported symbols of the one row
layout (the capacity signatures under the unsuffixed names)."""
import ctypes

import pytest
import torch

CAP_SYMBOLS = ('sug_grid_subsample', 'sug_radius_neighbors', 'sug_radius_reverse', 'sug_kpconv_fwd',
               'sug_seg_instnorm_fwd', 'sug_seg_instnorm_bwd', 'sug_seg_mean_fwd', 'sug_seg_mean_bwd',
               'sug_kp_sample_rows')


def test_level_capacity_arithmetic():
    from sug_amd.model.KPConv_model import level_capacity
    # the golden batch: B = 4, N = 1024, caps (976, 656, 256, 80)
    assert level_capacity(4, 1024, (976, 656, 256, 80)) == [4096, 3904, 2624, 1024, 320]
    # rounded up to a multiple of 64 rows
    assert level_capacity(4, 256, (250, 205, 65, 9)) == [1024, 1024, 832, 320, 64]
    assert level_capacity(3, 100, (33.4, 1, 1, 1)) == [300, 128, 64, 64, 64]
    # never above the level before (no cloud grows), C_0 = B*N exactly even when it is no multiple of 64
    assert level_capacity(2, 50, (1000, 1000, 7, 1000)) == [100, 100, 100, 64, 64]
    assert level_capacity(1, 10, ()) == [10]


def test_set_level_caps_validation_and_flag():
    from sug_amd.model.Model import Net_MDA, KPConv_g
    from sug_amd.model.KPConv_model import KPFCls
    assert KPConv_g.graph_capturable is False and KPFCls.graph_capturable is False        # the defaults stay
    for m in (Net_MDA('KPConv').g, KPFCls()):
        assert m.graph_capturable is False and m.level_caps is None
        for bad in ((1, 2, 3), (1, 2, 3, 4, 5), (1, 2, 0, 4), (1, -2, 3, 4), (1, 2, float('nan'), 4), (1, 2, float('inf'), 4),
                    (1, 2, '3', 4), (True, 2, 3, 4), 7, 'abcd'):
            with pytest.raises(ValueError):
                m.set_level_caps(bad)
            assert m.graph_capturable is False and m.level_caps is None                  # a refused call changes nothing
        m.set_level_caps([976, 656.5, 256, 80])
        assert m.graph_capturable is True
        assert m.level_caps == (976, 656.5, 256, 80) and m.preprocessor.level_caps == m.level_caps
        m.set_level_caps(None)
        assert m.graph_capturable is False and m.level_caps is None and m.preprocessor.level_caps is None
        with pytest.raises(RuntimeError, match='set_level_caps'):
            m.capacity_report()


def test_caps_leave_the_state_dict_alone():
    from sug_amd.model.KPConv_model import KPFCls
    m = KPFCls()
    keys = list(m.state_dict().keys())
    m.set_level_caps((10, 10, 10, 10))
    assert list(m.state_dict().keys()) == keys


def test_sugstep_follows_the_caps():
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import SUGStep
    m = Net_MDA('KPConv')
    with pytest.raises(NotImplementedError, match='set_level_caps'):
        SUGStep(m)
    m.g.set_level_caps((976, 656, 256, 80))
    st = SUGStep(m)                                         # accepted (on the CPU nothing can run: construction only)
    assert st.pair_domains
    m.g.set_level_caps(None)
    with pytest.raises(NotImplementedError, match='four-call'):
        SUGStep(m)


def test_uda_step_and_call_graphs_keep_declining():
    from sug_amd import call_graphs
    from sug_amd.model.Model import Net_MDA
    from sug_amd.uda_step import UDAStep
    m = Net_MDA('KPConv')
    m.g.set_level_caps((976, 656, 256, 80))
    assert call_graphs.manager_for(m) is None
    st = UDAStep(m, use_graph=True)
    assert not st.use_graph and not st.pair_domains       # (the reason string: tests/test_gpu_kpconv_caps.py)


def test_report_before_any_forward_and_overflow_message():
    from sug_amd.model.KPConv_model import KPFCls
    from sug_amd.train_step import check_level_caps
    m = KPFCls()
    assert check_level_caps(m) is None                      # no caps: nothing to read
    m.set_level_caps((8, 8, 8, 8))
    rep = m.capacity_report()
    assert rep['overflows'] == 0 and [l['level'] for l in rep['levels']] == [1, 2, 3, 4]
    assert all(l['needed'] == 0 for l in rep['levels'])
    # the epoch read's message, from a record as the device would leave it (B = 4, N = 256: capacity 64 rows at level 3)
    pre = m.preprocessor
    pre._shape = (4, 256)
    pre._record = torch.tensor([30, 28, 811, 40, 2, 1, 0, 0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r'level 3 needed 811 rows \(capacity 64\): a cap of 203 rows per cloud'):
        check_level_caps(m, reset=True)
    assert int(pre._record.abs().sum()) == 0                # reset cleared it
    assert check_level_caps(m)['overflows'] == 0


def test_capacity_symbols_declared_and_exported():
    from sug_amd import _lib
    for name in CAP_SYMBOLS:
        assert name in _lib.SIGNATURES, name
    assert _lib.CONSTANTS['SUG_KPCONV_RECORD_INTS'] == 8
    assert _lib.CONSTANTS['SUG_ABI_VERSION'] == 8           # signatures changed, the *_cap twins are gone
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in CAP_SYMBOLS:
        assert hasattr(L, name), name
        if name != 'sug_kp_sample_rows':
            assert name + '_cap' not in _lib.SIGNATURES and not hasattr(L, name + '_cap'), name
    # bad arguments are refused on the host, before any launch
    p = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    B = _lib.lib()
    assert B.sug_grid_subsample(p, p, 2, 8, 0.1, 17, 0, p, p, p, p, p, None) != 0      # capacity above B*cap
    assert B.sug_grid_subsample(p, p, 2, 8, 0.1, 16, 4, p, p, p, p, p, None) != 0      # level outside the record
    assert b'level 4 outside' in B.sug_last_error()
    assert B.sug_kpconv_fwd(p, p, p, None, 8, 4, 8, p, 15, 0.1, p, 4, p, p, p, None) != 0   # no valid-count pointer
    # a null record with any level passes the argument check: the refusal is the NEXT check's (dl, which nothing launches)
    assert B.sug_grid_subsample(p, p, 2, 8, 0.0, 16, 7, p, p, p, p, None, None) == _lib.CONSTANTS['SUG_ERR_ARG']
    assert b'dl must be positive' in B.sug_last_error()
    assert B.sug_grid_subsample(p, p, 2, 8, 0.0, 16, 7, p, p, p, p, p, None) != 0
    assert b'level 7 outside' in B.sug_last_error()


def test_capacity_ops_refuse_cpu_tensors():
    from sug_amd import ops
    x = torch.zeros(8, 4)
    p = torch.zeros(8, 3)
    off = torch.tensor([0, 8], dtype=torch.int32)
    nbr = torch.zeros(8, 4, dtype=torch.int32)
    rec = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.kp_grid_subsample(p, off, 1, 8, 0.1, 8, rec, 0)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.radius_neighbors(p, off, p, off, 0.1, 4)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.radius_reverse(nbr, off, off, 8, 8)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.kpconv(x, p, p, nbr, None, torch.zeros(15, 3), torch.zeros(15, 4, 4), 0.02, off)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.seg_instnorm(x, off, act=True)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.seg_mean(x, off)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.kp_sample_rows(x, off)
