"""CPU: the part-segmentation loader -- the header's declaration and constants, the refusals sug_prepare_seg_batch makes on the
host before any launch, pack_clouds, PartSegDataset's construction-time checks, and the host restatement of the fill draw
(trusted here before tests/test_gpu_seg_loader.py compares the GPU with it)."""
import ctypes

import numpy as np
import pytest
import torch

import seg_cases as S
import seg_loader_cases as SL


# ------------------------------------------------------------------------------------------------ binding
def test_header_declares_the_entry_point_and_constants():
    from sug_amd import _lib, ops
    from sug_amd._lib import SIGNATURES, DECLARATIONS, _vp, _i32, _f32
    H = _lib.CONSTANTS
    assert H['SUG_ABI_VERSION'] == 8
    assert (H['SUG_PREP_NORMALS'], H['SUG_PREP_DRAW_FILL'], H['SUG_PREP_SEG_MAX_EXTRA']) == (128, 0x60000000, 8)
    assert (ops.PREP_NORMALS, ops.PREP_SEG_MAX_EXTRA) == (128, 8)
    old = [H['SUG_PREP_' + n] for n in ('NORMALIZE', 'ROTATE_Z', 'JITTER', 'SHUFFLE', 'SCALE', 'PERTURB', 'SHIFT')]
    assert old == [1, 2, 4, 8, 16, 32, 64], 'the old stage bits moved'
    assert [H['SUG_PREP_DRAW_' + n] >> 28 for n in ('ANGLE', 'SUBSET', 'NOISE', 'SCALE', 'PERTURB', 'SHIFT', 'FILL')] == list(range(7))
    # written by hand from the prototype: pts extra point_label category lengths | M P E | idx | B N stages | pre_rot angles noise
    # sel scales perturb shifts | seed | counter | sigma clip | aug_params out label_out category_out, six draws out, stream
    want = [_vp] * 5 + [_i32] * 3 + [_vp] + [_i32] * 3 + [_vp] * 7 + [ctypes.c_uint64] + [_vp] + [_f32] * 2 + [_vp] * 11
    assert SIGNATURES['sug_prepare_seg_batch'] == want
    assert DECLARATIONS['sug_prepare_seg_batch'][0] is ctypes.c_int
    assert hasattr(_lib.lib(), 'sug_prepare_seg_batch')


# ------------------------------------------------------------------------------------------------ refusals on the host
def _err():
    from sug_amd import _lib
    return _lib.lib().sug_last_error().decode()


def _call(**kw):
    """sug_prepare_seg_batch on dummy host buffers (every case below is refused before a pointer is used); kw overrides."""
    from sug_amd import _lib, ops
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    params = (ctypes.c_float * 5)(0.8, 1.25, 0.1, 0.06, 0.18)
    a = dict(pts=p, extra=p, point_label=p, category=p, lengths=p, M=4, P=96, E=3, idx=p, B=2, N=64, stages=ops.PREP_NORMALIZE,
             pre_rot=None, angles=None, noise=None, sel=None, scales=None, perturb=None, shifts=None, seed=1, counter=p,
             sigma=0.01, clip=0.05, aug_params=params, out=p, label_out=p, category_out=p, angles_out=None, noise_out=None,
             sel_out=None, scales_out=None, perturb_out=None, shifts_out=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.lib().sug_prepare_seg_batch(*a.values())


@pytest.mark.parametrize('kw, text', [
    (dict(pts=None), 'null pointer'), (dict(idx=None), 'null pointer'), (dict(out=None), 'null pointer'),
    (dict(label_out=None), 'null pointer'), (dict(point_label=None), 'null pointer'),
    (dict(extra=None), 'null extra with E=3'),
    (dict(E=-1), 'E=-1'), (dict(E=9), 'E=9'),
    (dict(stages=128, E=2), 'SUG_PREP_NORMALS needs E >= 3'), (dict(stages=128, E=0, extra=None), 'SUG_PREP_NORMALS needs E >= 3'),
    (dict(B=0), 'B=0'), (dict(M=0), 'M=0'), (dict(P=0), 'P=0'), (dict(N=0), 'N=0'),
    (dict(P=4097), 'P=4097'), (dict(N=4097), 'N=4097'),
    (dict(stages=256), 'unknown bits in stages=256'), (dict(stages=-1), 'unknown bits'),
    (dict(stages=16, aug_params=None), 'null aug_params'),
    (dict(stages=16, aug_params=(ctypes.c_float * 5)(1.25, 0.8, 0.1, 0.06, 0.18)), 'scale_low'),
    (dict(stages=16, aug_params=(ctypes.c_float * 5)(0.0, 0.8, 0.1, 0.06, 0.18)), 'scale_low'),
    (dict(stages=64, aug_params=(ctypes.c_float * 5)(0.8, 1.25, -0.1, 0.06, 0.18)), 'shift_range'),
    (dict(stages=64, aug_params=(ctypes.c_float * 5)(0.8, 1.25, float('inf'), 0.06, 0.18)), 'shift_range'),
    (dict(stages=32, aug_params=(ctypes.c_float * 5)(0.8, 1.25, 0.1, -1.0, 0.18)), 'angle_sigma'),
    (dict(stages=32, aug_params=(ctypes.c_float * 5)(0.8, 1.25, 0.1, 0.06, float('nan'))), 'angle_clip'),
    (dict(counter=None), 'null counter'),                                   # no sel: the subset or the fill is drawn
    (dict(counter=None, sel='p', stages=2), 'null counter'),                # sel given, but the angle is drawn
    (dict(counter=None, sel='p', stages=4), 'null counter'),
    (dict(counter=None, sel='p', stages=16), 'null counter'),
    (dict(counter=None, sel='p', stages=32), 'null counter'),
    (dict(counter=None, sel='p', stages=64), 'null counter'),
    (dict(sigma=-1.0), 'sigma and clip'),
])
def test_refused_on_the_host_before_a_launch(kw, text):
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    kw = {k: (p if isinstance(v, str) else v) for k, v in kw.items()}
    assert _call(**kw) == -1
    msg = _err()
    assert msg.startswith('sug_prepare_seg_batch:') and text in msg, msg


def test_cpu_tensors_raise_the_hip_device_message():
    from sug_amd import ops
    c = SL.make_case('small')
    t = {k: torch.as_tensor(c[k]) for k in ('pts', 'extra', 'point_label', 'category', 'lengths')}
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.prepare_seg_batch(t['pts'], t['extra'], t['point_label'], t['category'], t['lengths'],
                              torch.arange(2, dtype=torch.int32), 64)


# ------------------------------------------------------------------------------------------------ pack_clouds
def test_pack_clouds_on_a_ragged_list():
    from sug_amd.data import pack_clouds
    r = np.random.RandomState(0)
    clouds = [r.rand(n, 6).astype(np.float32) for n in (5, 9, 1)]
    packed, lengths = pack_clouds(clouds)
    assert packed.shape == (3, 9, 6) and packed.dtype == np.float32
    assert lengths.dtype == np.int32 and lengths.tolist() == [5, 9, 1]
    for m, c in enumerate(clouds):
        assert np.array_equal(packed[m, :len(c)], c) and not packed[m, len(c):].any()
    labels, l2 = pack_clouds([np.arange(n, dtype=np.int64) % 4 for n in (5, 9, 1)])
    assert labels.shape == (3, 9) and labels.dtype == np.int64 and l2.tolist() == [5, 9, 1]
    assert labels[0].tolist() == [0, 1, 2, 3, 0, 0, 0, 0, 0]
    tens, l3 = pack_clouds([torch.ones(2, 3), torch.ones(4, 3)])                # tensors are taken too
    assert tens.shape == (2, 4, 3) and l3.tolist() == [2, 4]
    with pytest.raises(ValueError, match='cloud 1'):
        pack_clouds([r.rand(5, 6), r.rand(5, 3)])
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        pack_clouds([r.rand(5, 6), r.rand(0, 6)])
    with pytest.raises(ValueError, match='empty list'):
        pack_clouds([])


# ------------------------------------------------------------------------------------------------ PartSegDataset
def _good(M=4, P=20):
    r = np.random.RandomState(1)
    pts = r.rand(M, P, 6).astype(np.float32)
    cat = np.array([0, 1, 2, 0][:M])
    lab = np.stack([S.PART_FIRST[k] + r.randint(0, S.PART_COUNT[k], P) for k in cat])
    return pts, lab, cat


def _make(pts, lab, cat, **kw):
    from sug_amd.data import PartSegDataset
    return PartSegDataset(pts, lab, cat, S.PART_FIRST, S.PART_COUNT, num_points=16, **kw)


def test_dataset_value_errors_name_the_first_offender():
    from sug_amd import ops
    pts, lab, cat = _good()
    with pytest.raises(ValueError, match=r'cloud 2 has length 0, outside \[1, P = 20\]'):
        _make(pts, lab, cat, lengths=[20, 3, 0, 21])
    with pytest.raises(ValueError, match=r'cloud 3 has length 21'):
        _make(pts, lab, cat, lengths=[20, 3, 1, 21])
    big = np.zeros((1, ops.PREP_MAX_POINTS + 1, 3), np.float32)
    with pytest.raises(ValueError, match='at most %d points per cloud, got %d' % (ops.PREP_MAX_POINTS, ops.PREP_MAX_POINTS + 1)):
        _make(big, np.zeros(big.shape[:2], np.int64), np.zeros(1, np.int64))
    for wrong in (3, -1):
        c2 = cat.copy()
        c2[1] = wrong
        with pytest.raises(ValueError, match=r'cloud 1 has category %d, outside \[0, K = 3\)' % wrong):
            _make(pts, lab, c2)
    l2 = lab.copy()
    l2[1, 7] = 4                                                  # category 1 owns part 3 alone
    l2[2, 0] = 0
    with pytest.raises(ValueError, match=r'label 4 of point 7 of cloud 1 \(category 1: parts \[3, 4\)\) is outside the part range'):
        _make(pts, l2, cat)
    l3 = lab.copy()
    l3[3, 19] = 64
    with pytest.raises(ValueError, match='label 64 of point 19 of cloud 3 .* is not below SUG_SEG_MAX_PARTS = 64'):
        _make(pts, l3, cat)
    with pytest.raises(ValueError, match='point_labels must be'):
        _make(pts, lab[:, :10], cat)
    with pytest.raises(ValueError, match="'dropout'"):
        _make(pts, lab, cat, aug={'dropout': 0.5})
    with pytest.raises(ValueError, match='extra channels'):
        _make(np.zeros((4, 20, 12), np.float32), lab, cat)
    # a list whose points and labels differ in length
    with pytest.raises(ValueError, match='cloud 1: its points and its labels differ in length'):
        _make([pts[0, :5], pts[1, :9]], [lab[0, :5], lab[1, :8]], cat[:2])


def test_dataset_ignores_labels_behind_a_clouds_length():
    """A bad label in a padding row is not an offender; the first check to fail is then the device's."""
    pts, lab, cat = _good()
    lab[1, 12:] = 63
    with pytest.raises(ValueError, match='label 63 of point 12 of cloud 1'):
        _make(pts, lab, cat)
    with pytest.raises(RuntimeError, match='HIP device'):
        _make(pts, lab, cat, lengths=[20, 12, 20, 20], device='cpu')


def test_dataset_refuses_a_cpu_device():
    pts, lab, cat = _good()
    with pytest.raises(RuntimeError, match='HIP device only .*no CPU fallback'):
        _make(pts, lab, cat, device='cpu')
    with pytest.raises(RuntimeError, match='HIP device'):
        _make(torch.as_tensor(pts), lab, cat, device=torch.device('cpu'))


# ------------------------------------------------------------------------------------------------ the fill draw
def test_fill_sources_by_hand():
    # (word * L) >> 32: 0 -> 0; 2^31 -> L / 2; the largest word -> L - 1; 2^32 / 5 = 858993459.2: the step from 0 to 1 at L = 5
    assert SL.fill_sources([0, 0x80000000, 0xFFFFFFFF, 858993459, 858993460], 5).tolist() == [0, 2, 4, 0, 1]
    assert SL.fill_sources([0x80000000, 0xFFFFFFFF], 4096).tolist() == [2048, 4095]
    assert SL.fill_sources([0xFFFFFFFF, 0x12345678], 1).tolist() == [0, 0]
    # the first block of the fill purpose at (SEED, counter 5, slot 0), worked by hand from its four words at L = 5:
    # 0x95f8d887 / 2^32 * 5 = 2.93, 0x435f28e2 -> 1.32, 0xdb90715b -> 4.29, 0x07238d90 -> 0.14
    import data_pipeline_cases as C
    words = C._words(SL.SEED, 5, 1, SL.DRAW_FILL, 1)[0, 0]
    assert [int(w) for w in words] == [0x95f8d887, 0x435f28e2, 0xdb90715b, 0x07238d90]
    assert SL.host_fill(SL.SEED, 5, 0, 5, 16).tolist() == [2, 1, 4, 0, 4, 1, 0, 3, 0, 2, 2]


@pytest.mark.parametrize('L, N', [(5, 64), (41, 64), (64, 64), (130, 256), (2500, 2048), (1, 9)])
def test_host_fill_is_well_formed(L, N):
    for b in (0, 3):
        f = SL.host_fill(SL.SEED, 7, b, L, N)
        assert f.shape == (max(N - L, 0),) and f.dtype == np.int32
        assert (f >= 0).all() and (f < L).all()
        src = SL.host_sources(SL.SEED, 7, b, L, N)
        assert src.shape == (N,) and (src >= 0).all() and (src < L).all()
        if L <= N:
            assert src[:L].tolist() == list(range(L)) and np.array_equal(src[L:], f)
        else:
            assert len(set(src.tolist())) == N                  # a subset: no repeats
    # a partial last block is the prefix of the full one, and the slots draw differently
    if N - L > 5:
        assert np.array_equal(SL.host_fill(SL.SEED, 7, 0, L, N)[:5], SL.host_fill(SL.SEED, 7, 0, L, L + 5))
    if L > 1 and N - L >= 16:
        assert not np.array_equal(SL.host_fill(SL.SEED, 7, 0, L, N), SL.host_fill(SL.SEED, 7, 3, L, N))
        assert not np.array_equal(SL.host_fill(SL.SEED, 7, 0, L, N), SL.host_fill(SL.SEED, 8, 0, L, N))
