"""CPU: part segmentation -- the numpy restatement of the ShapeNet-Part IoU protocol against hand-worked numbers (it has no
reference, so it is trusted here before tests/test_gpu_seg.py compares the GPU with it), the layout of Pointnet2PartSeg,
the header's constants and signatures, and the refusals the library makes on the host before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import pn2_msg_fp_cases as C
import seg_cases as S


# ------------------------------------------------------------------------------------------------ the IoU restatement
def test_iou_restatement_on_the_hand_worked_clouds():
    """Cloud 0, parts {0, 1, 2}: label 0 on points 0-3 and 1 on points 4-7, prediction 0 on points 0, 1, 2, 7 and 1 on points
    3-6 (points 0 and 4 by the lowest index of a tie; column 5, the global maximum, is outside the range and ignored):
    part 0: I = 3, U = 4 + 4 - 3 = 5; part 1: I = 3, U = 5; part 2 absent from both: 1 by rule -> (0.6 + 0.6 + 1) / 3.
    Cloud 1, the one-part category: I = U = 8 -> 1.  Cloud 2, parts {4, 5}: label 4 on points 0-5, prediction 4 on points 0-2:
    part 4: I = 3, U = 6; part 5: I = 2, U = 5 -> (0.5 + 0.4) / 2."""
    z, lab, cat = S.hand_case()
    bk = S.part_iou_books(z, lab, cat, S.PART_FIRST, S.PART_COUNT)
    assert (bk['shapes'], bk['points'], bk['correct'], bk['error']) == (3, 24, 6 + 8 + 5, 0)
    np.testing.assert_allclose(bk['cat_iou'], [(0.6 + 0.6 + 1.0) / 3, 1.0, 0.45], rtol=1e-15)
    assert bk['cat_iou'][0] == pytest.approx(0.7333333333333333, rel=1e-15)
    assert bk['cat_shapes'].tolist() == [1, 1, 1]
    assert bk['part_points'].tolist() == [4, 4, 0, 8, 6, 2]
    assert bk['part_correct'].tolist() == [3, 3, 0, 8, 3, 2]


def test_iou_restatement_single_cloud_of_eight_points():
    """The first cloud alone, and the books continued over a second call."""
    z, lab, cat = S.hand_case()
    bk = S.part_iou_books(z[:1], lab[:1], cat[:1], S.PART_FIRST, S.PART_COUNT)
    assert (bk['shapes'], bk['points'], bk['correct']) == (1, 8, 6)
    assert bk['cat_iou'].tolist() == [(0.6 + 0.6 + 1.0) / 3, 0.0, 0.0]
    bk = S.part_iou_books(z[1:], lab[1:], cat[1:], S.PART_FIRST, S.PART_COUNT, bk)
    whole = S.part_iou_books(z, lab, cat, S.PART_FIRST, S.PART_COUNT)
    for k in whole:
        assert np.array_equal(bk[k], whole[k]), k


def test_iou_restatement_ties_and_the_maximum_outside_the_range():
    # one cloud of 2 points in category 2 (parts {4, 5}): a tie between 4 and 5 -> 4; column 0 holds 100 and is not looked at
    z = np.array([[[100.0, 0, 0, 0, 2.0, 2.0], [100.0, 0, 0, 0, -1.0, -0.5]]], np.float32)
    bk = S.part_iou_books(z, np.array([[4, 4]]), np.array([2]), S.PART_FIRST, S.PART_COUNT)
    # prediction (4, 5): part 4: I = 1, U = 2; part 5: I = 0, U = 1 -> (0.5 + 0) / 2
    assert bk['cat_iou'].tolist() == [0.0, 0.0, 0.25] and bk['correct'] == 1
    assert bk['part_points'].tolist() == [0, 0, 0, 0, 2, 0] and bk['part_correct'].tolist() == [0, 0, 0, 0, 1, 0]


def test_iou_restatement_does_not_score_a_bad_cloud():
    z, lab, cat = S.hand_case()
    want = S.part_iou_books(z[1:], lab[1:], cat[1:], S.PART_FIRST, S.PART_COUNT)
    lab = lab.copy()
    lab[0, 3] = 3                                # a label outside category 0's range
    bk = S.part_iou_books(z, lab, cat, S.PART_FIRST, S.PART_COUNT)
    assert bk['error'] == 1
    bk2 = S.part_iou_books(z, S.hand_case()[1], np.array([3, 1, 2]), S.PART_FIRST, S.PART_COUNT)        # category == K
    for b in (bk, bk2):
        for k in want:
            if k != 'error':
                assert np.array_equal(b[k], want[k]), k


# ------------------------------------------------------------------------------------------------ model layout
@pytest.mark.parametrize('extra', [0, 3])
def test_model_layout_and_restated_state_dict(extra):
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    net = Pointnet2PartSeg(num_part=50, num_category=16, extra_channels=extra)
    sd = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    base = {k: tuple(v.shape) for k, v in C.SegNet(C.Restated).state_dict().items()}
    changed = {'fp1.mlp_convs.0.weight': (128, 128 + 16 + 3 + extra, 1)}
    if extra:
        changed.update({'sa1.conv_blocks.%d.0.weight' % i: (w, 3 + extra, 1, 1) for i, w in enumerate((32, 64, 64))})
    for k, shape in base.items():
        assert sd[k] == changed.get(k, shape), k
    head = {'conv1.weight': (128, 128, 1), 'conv1.bias': (128,), 'bn1.weight': (128,), 'bn1.bias': (128,),
            'bn1.running_mean': (128,), 'bn1.running_var': (128,), 'bn1.num_batches_tracked': (),
            'conv2.weight': (50, 128, 1), 'conv2.bias': (50,)}
    assert {k: v for k, v in sd.items() if k not in base} == head
    assert isinstance(net.drop1, torch.nn.Dropout) and net.drop1.p == 0.5
    # a state dict of the restated model loads with strict=True
    ref = S.SegPartNet(num_part=50, num_category=16, extra_channels=extra)
    net.load_state_dict(C.load_seeded(ref, 7), strict=True)
    assert list(net.state_dict()) == list(ref.state_dict())


def test_reference_runs_agree_on_every_index_list():
    """The seed of the GPU model test: the restatement's fp32 and fp64 runs take the same FPS draws, ball-query and 3-NN
    lists (asserted inside reference_runs)."""
    for extra in (0, 3):
        r32, r64, lists = S.reference_runs('train', extra)
        assert len(lists) == 2 + 3 + 2 + 2 and r32['grad_names'] == r64['grad_names']
        assert abs(r32['loss'] - r64['loss']) < 1e-4


# ------------------------------------------------------------------------------------------------ header
def test_header_constants_and_abi_version():
    from sug_amd import _lib, ops
    H = _lib.CONSTANTS
    assert H['SUG_ABI_VERSION'] == 8
    assert H['SUG_POINT_CE_MAX_ROWS'] >= 1 << 22 and H['SUG_POINT_CE_MAX_CLASSES'] == 64
    assert H['SUG_POINT_CE_BLOCK_ROWS'] == ops.POINT_CE_BLOCK_ROWS >= 64
    assert H['SUG_SEG_MAX_PARTS'] == 64 and H['SUG_SEG_MAX_CATEGORIES'] == 64
    assert H['SUG_SEG_MAX_CATEGORY_PARTS'] >= 8 and H['SUG_SEG_MAX_CLOUDS'] >= 256
    assert H['SUG_SEG_RECORD_WORDS'] >= 8 + 2 * H['SUG_SEG_MAX_CATEGORY_PARTS']
    # the state block: four totals, then four arrays of 64 words that do not overlap
    assert (H['SUG_SEG_SHAPES'], H['SUG_SEG_POINTS'], H['SUG_SEG_CORRECT'], H['SUG_SEG_ERROR']) == (0, 1, 2, 3)
    offs = [H['SUG_SEG_' + n] for n in ('CAT_IOU', 'CAT_SHAPES', 'PART_POINTS', 'PART_CORRECT')] + [H['SUG_SEG_STATE_WORDS']]
    assert offs[0] >= 4 and all(b - a >= 64 for a, b in zip(offs[:-1], offs[1:]))
    st = ops.part_iou_state('cpu')
    assert st.shape == (H['SUG_SEG_STATE_WORDS'],) and st.dtype == torch.int64 and not st.any()


def test_ctypes_signatures_match_header():
    """The binding is derived from the header; these lists are written by hand from the four prototypes."""
    from sug_amd._lib import SIGNATURES, DECLARATIONS, _vp, _i32, _i64
    assert SIGNATURES['sug_point_ce_workspace'] == [_i32]
    assert SIGNATURES['sug_point_ce_fwd'] == [_vp, _i64, _vp, _i32, _i32, _i64] + [_vp] * 7
    #                                         logits ld label M C ignore_index | class_weight loss lse pred workspace totals stream
    assert SIGNATURES['sug_point_ce_bwd'] == [_vp, _i64, _vp, _i32, _i32, _i64] + [_vp] * 5
    #                                         ... | class_weight g lse dlogits stream
    assert SIGNATURES['sug_part_iou_accumulate'] == [_vp] * 5 + [_i32] * 4 + [_vp] * 3
    for n in ('sug_point_ce_workspace', 'sug_point_ce_fwd', 'sug_point_ce_bwd', 'sug_part_iou_accumulate'):
        assert DECLARATIONS[n][0] is ctypes.c_int


# ------------------------------------------------------------------------------------------------ refusals on the host
def _buf():
    return ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)


def _err():
    from sug_amd import _lib
    return _lib.lib().sug_last_error().decode()


@pytest.mark.parametrize('M, Cn', [(0, 10), (8, 1), (8, 65)])
def test_point_ce_shape_is_refused_before_a_launch(M, Cn):
    from sug_amd import _lib
    L, p = _lib.lib(), _buf()
    assert L.sug_point_ce_fwd(p, Cn, p, M, Cn, -100, None, p, p, None, p, None, None) == -1
    assert 'sug_point_ce_fwd' in _err() and 'M=%d rows, C=%d classes' % (M, Cn) in _err()
    assert L.sug_point_ce_bwd(p, Cn, p, M, Cn, -100, None, p, p, p, None) == -1
    assert 'sug_point_ce_bwd' in _err()


def test_point_ce_workspace_and_row_limits():
    from sug_amd import _lib
    L, H, p = _lib.lib(), _lib.CONSTANTS, _buf()
    R, W = H['SUG_POINT_CE_BLOCK_ROWS'], H['SUG_POINT_CE_PARTIAL_WORDS']
    assert [L.sug_point_ce_workspace(m) for m in (1, R, R + 1, 2 * R + 1)] == [W, W, 2 * W, 3 * W]
    big = H['SUG_POINT_CE_MAX_ROWS'] + 1
    assert L.sug_point_ce_workspace(0) == -1 and L.sug_point_ce_workspace(big) == -1 and 'sug_point_ce_workspace' in _err()
    assert L.sug_point_ce_fwd(p, 10, p, big, 10, -100, None, p, p, None, p, None, None) == -1 and 'sug_point_ce_fwd' in _err()
    assert L.sug_point_ce_fwd(p, 9, p, 8, 10, -100, None, p, p, None, p, None, None) == -1 and 'ld=9' in _err()
    assert L.sug_point_ce_fwd(p, 10, p, 8, 10, -100, None, p, None, None, p, None, None) == -1 and 'null' in _err()


def test_part_iou_limits_are_refused_before_a_launch():
    from sug_amd import _lib
    L, H, p = _lib.lib(), _lib.CONSTANTS, _buf()
    first, count = (ctypes.c_int32 * 65)(*([0] * 65)), (ctypes.c_int32 * 65)(*([1] * 65))
    call = lambda B, N, Cn, K: L.sug_part_iou_accumulate(p, p, p, first, count, B, N, Cn, K, p, p, None)
    assert call(2, 8, 6, 65) == -1 and 'sug_part_iou_accumulate' in _err() and 'K=65' in _err()
    assert call(2, 8, 65, 3) == -1 and 'C=65' in _err()
    assert call(0, 8, 6, 3) == -1 and call(2, 0, 6, 3) == -1 and call(H['SUG_SEG_MAX_CLOUDS'] + 1, 8, 6, 3) == -1
    top = H['SUG_SEG_MAX_CATEGORY_PARTS']
    count[1] = top + 1                                          # a part_count above the limit
    assert call(2, 8, 64, 3) == -1 and 'sug_part_iou_accumulate: category 1' in _err() and str(top) in _err()
    count[1], first[2] = 2, 5                                   # a range that leaves the logits' columns: [5, 7) of C = 6
    count[2] = 2
    assert call(2, 8, 6, 3) == -1 and 'category 2' in _err()
    first[2] = -1
    assert call(2, 8, 6, 3) == -1 and 'category 2' in _err()


def test_cpu_tensors_raise_the_hip_device_message():
    from sug_amd import ops
    from sug_amd.model.pointnet2_seg import Pointnet2PartSeg
    from sug_amd.utils.seg_utils import PartIoUMeter
    z, lab = torch.zeros(2, 8, 6), torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.point_ce(z, lab)
    assert not ops.point_ce_supported(z, lab)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.part_iou_accumulate(z, lab, torch.zeros(2, dtype=torch.int64), S.PART_FIRST, S.PART_COUNT,
                                torch.zeros(ops.SEG_STATE_WORDS, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='HIP device'):
        Pointnet2PartSeg(num_part=8, num_category=3, npoint1=64, npoint2=16)(torch.zeros(2, 3, 256), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='HIP device'):
        PartIoUMeter(S.PART_FIRST, S.PART_COUNT, 'cpu')
