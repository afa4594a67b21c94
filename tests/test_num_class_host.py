"""Class counts other than ten, the host side: the public interface takes `num_class` (Net_MDA, the mirrored functions of
model/mmd.py, the step drivers, UnifiedPointDG's class lists), the defaults are what they were, and the fp64 restatement
tests/num_class_cases.py that the GPU tests compare against is pinned at ten classes against the oracle."""
import pytest
import torch

import num_class_cases as NC
from oracle import ref_cpu as O

BACKBONES = ('Pointnet', 'Pointnet2', 'DGCNN', 'PTran', 'KPConv')


@pytest.mark.parametrize('name', BACKBONES)
def test_default_state_dict_is_unchanged(name):
    from sug_amd.model.Model import Net_MDA
    a = {k: tuple(v.shape) for k, v in Net_MDA(name).state_dict().items()}
    b = {k: tuple(v.shape) for k, v in Net_MDA(name, num_class=10).state_dict().items()}
    assert list(a.items()) == list(b.items())
    assert a['c1.mlp3.weight'][0] == a['c2.mlp3.weight'][0] == 10


@pytest.mark.parametrize('name', BACKBONES)
def test_num_class_sets_both_heads(name):
    from sug_amd.model.Model import Net_MDA
    net = Net_MDA(name, num_class=11)
    assert net.c1.mlp3.out_features == net.c2.mlp3.out_features == 11
    assert net.c1.mlp3.in_features == Net_MDA(name).c1.mlp3.in_features


@pytest.mark.parametrize('bad', [1, 0, -3, 2.5])
def test_num_class_below_two_is_refused(bad):
    from sug_amd.model.Model import Net_MDA
    with pytest.raises(ValueError, match='num_class'):
        Net_MDA('Pointnet', num_class=bad)


def test_head_linear_supported_widths():
    from sug_amd import _lib
    L = _lib.lib()
    assert [L.sug_head_linear_supported(8, 256, No, 1, 0) for No in (10, 32, 40, 64)] == [1, 1, 1, 1]
    assert [L.sug_head_linear_supported(8, 256, No, 1, 0) for No in (33, 42, 68)] == [0, 0, 0]
    # 33..64 is a last layer's width only (no epilogue); the hidden widths answer as before
    assert L.sug_head_linear_supported(8, 1024, 40, 0, 1) == 0
    assert [L.sug_head_linear_supported(8, 1024, No, 0, 1) for No in (256, 512)] == [1, 1]
    assert [L.sug_head_linear_supported(8, 512, No, 1, 1) for No in (256, 512)] == [1, 1]
    assert [L.sug_head_linear_supported(8, 256, No, 1, 0) for No in (256, 512, 128)] == [1, 1, 0]
    assert L.sug_head_linear_supported(129, 256, 40, 1, 0) == 0 and L.sug_head_linear_supported(8, 300, 40, 1, 0) == 0


def test_class_lists_and_weights_for_fifteen_classes():
    from sug_amd.data import dataloader as D
    labels = [14, 0, 3, 14, 7, 3, 3] + list(range(15))
    idx = D.class_indices(labels, 15)
    assert len(idx) == 15 and idx[14] == [0, 3, 21] and idx[3] == [2, 5, 6, 10] and all(idx)
    assert D.class_indices([0, 1], 10) == D.class_indices([0, 1])                    # the default is ten lists
    counts = [len(v) for v in idx]
    for weighting in ('number_inverse', 'exp_inverse', 'DLSA', 'uniform'):
        w = D.class_weights(counts, len(labels), weighting)
        assert len(w) == 15 and abs(sum(w) - 1.0) < 1e-6
    with pytest.raises(ValueError, match=r'label 15 .*15'):
        D.class_indices([0, 15], 15)
    with pytest.raises(ValueError, match=r'label 10 .*10'):
        D.class_indices([0, 10])
    with pytest.raises(ValueError, match=r'label -1 '):
        D.class_indices([0, -1], 15)


def test_mmd_cal_refuses_a_class_count_that_is_not_the_logits_width():
    """The check sits in prob_weights_soft in front of the device dispatch, so CPU tensors reach it (nothing here needs a
    GPU): an 11-class term without NUM_CLASS (the default, 10), and one that names 12."""
    from sug_amd.model import mmd
    g = torch.Generator().manual_seed(0)
    ps, pt = torch.randn(6, 11, generator=g), torch.randn(6, 11, generator=g)
    ls, lt = torch.randint(0, 11, (6,), generator=g), torch.randint(0, 11, (6,), generator=g)
    X, Y = torch.randn(6, 5, generator=g), torch.randn(6, 5, generator=g)
    cfg = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 5, 'SEM_WEIGHTS': 'mean2one', 'LABEL_WEIGHT': 0.5}
    with pytest.raises(ValueError, match=r'11 .*num_class is 10'):
        mmd.mmd_cal(ls, X, lt, Y, cfg, data_s=ps, data_t=pt)
    with pytest.raises(ValueError, match=r'11 .*num_class is 12'):
        mmd.mmd_cal(ls, X, lt, Y, dict(cfg, NUM_CLASS=12), data_s=ps, data_t=pt)
    with pytest.raises(ValueError, match=r'11 .*num_class is 10'):
        mmd.prob_weights_soft(ps, pt, ls, lt, 0.5, 'none')
    # the composed lines (CPU tensors) with the right count: the restatement's numbers
    for meth in NC.SDA_METHODS:
        got = mmd.prob_weights_soft(ps, pt, ls, lt, 0.5, meth, num_class=11)
        torch.testing.assert_close(got.double(), NC.sda_weights(ps, pt, ls, lt, 0.5, meth, 11), rtol=1e-4, atol=1e-7)
    got = mmd.cal_sample_weights(ps, pt, dict(cfg, NUM_CLASS=11), label_s=ls, label_t=lt)
    torch.testing.assert_close(got.double(), NC.sda_weights(ps, pt, ls, lt, 0.5, 'mean2one', 11), rtol=1e-4, atol=1e-7)


def test_class_pairs_host_and_overlap_take_the_count():
    from sug_amd.model import mmd
    from sug_amd.utils.common_utils import get_most_overlapped_element
    ls, lt = torch.tensor([10, 3, 10, 0]), torch.tensor([3, 10, 10, 10])
    assert mmd.class_pairs_host(ls, lt, 1) == ([1], [0])                              # ten classes: label 10 is never paired
    assert mmd.class_pairs_host(ls, lt, 1, num_class=11) == ([1, 0, 2], [0, 1, 2])
    with pytest.raises(AssertionError):
        get_most_overlapped_element(ls, lt)
    ind_s, ind_t = get_most_overlapped_element(ls, lt, num_class=11)
    assert sorted(ls[ind_s].tolist()) == sorted(lt[ind_t].tolist()) == [3, 10, 10]


def test_steps_take_the_class_count_from_the_model():
    from sug_amd.model.Model import Net_MDA
    from sug_amd.train_step import METHODS, SUGStep
    from sug_amd.uda_step import CLASS_MMD, UDAStep
    net = Net_MDA('Pointnet', num_class=11)
    tr = SUGStep(net)
    assert tr.num_class == 11
    assert tr.methods['GEO_MMD'][0]['NUM_CLASS'] == 11 and tr.methods['SEM_MMD'][0]['NUM_CLASS'] == 11
    assert 'NUM_CLASS' not in METHODS['GEO_MMD'][0] and 'NUM_CLASS' not in METHODS['SEM_MMD'][0]     # the step's own copies
    given = {'NAME': 'HARD_MMD', 'GEO_SCALE': 1}
    tr = SUGStep(net, methods={'GEO_MMD': [given], 'SEM_MMD': [{'NAME': 'HARD_MMD', 'SEM_SCALE': 1, 'NUM_CLASS': 11}]})
    assert tr.methods['GEO_MMD'][0]['NUM_CLASS'] == 11 and given == {'NAME': 'HARD_MMD', 'GEO_SCALE': 1}
    with pytest.raises(ValueError, match=r'NUM_CLASS 10 .* 11 classes'):
        SUGStep(net, methods={'SEM_MMD': [{'NAME': 'HARD_MMD', 'SEM_SCALE': 1, 'NUM_CLASS': 10}]})
    x = torch.zeros(2, 3, 8, 1)
    y = torch.zeros(2, dtype=torch.long)
    k11 = tr._graph_key(True, (x, y, x, y))
    k10 = SUGStep(Net_MDA('Pointnet'))._graph_key(True, (x, y, x, y))
    assert ('num_class', 11) in k11 and ('num_class', 10) in k10 and k11 != k10
    assert SUGStep(Net_MDA('Pointnet')).methods['SEM_MMD'][0]['NUM_CLASS'] == 10
    ud = UDAStep(net, 'naive_mmd')
    assert ud.num_class == 11 and ud.class_mmd == dict(CLASS_MMD, NUM_CLASS=11) and 'NUM_CLASS' not in CLASS_MMD
    assert ud._graph_key((x, y, x, y)) != UDAStep(Net_MDA('Pointnet'), 'naive_mmd')._graph_key((x, y, x, y))
    with pytest.raises(ValueError, match=r'NUM_CLASS 10 .* 11 classes'):
        UDAStep(net, 'naive_mmd', class_mmd={'NAME': 'HARD_MMD', 'NUM_CLASS': 10})


def test_source_only_classifiers_already_take_a_count():
    from sug_amd.model.model_pointnet import Pointnet_cls
    net = Pointnet_cls(num_class=15)
    widths = [m.out_features for m in net.modules() if isinstance(m, torch.nn.Linear)]
    assert widths[-1] == 15


@pytest.mark.parametrize('m', [5, 300])
def test_restatement_is_the_oracle_at_ten_classes(m):
    """tests/num_class_cases.py in fp64 against oracle.ref_cpu (fp32) at C = 10, rtol 1e-4: prob_weights_soft for the four
    weightings, soft_mmd with sample weights."""
    g = torch.Generator().manual_seed(40 + m)
    for seed in range(50):                      # 'mean2one' truncates 1 / mean: a draw whose fraction is safe in fp32 as well
        ps, pt = torch.randn(m, 10, generator=g) * 2, torch.randn(m, 10, generator=g) * 2
        ls, lt = torch.randint(0, 10, (m,), generator=g), torch.randint(0, 10, (m,), generator=g)
        if 0.05 <= NC.mean2one_fraction(ps, pt, ls, lt, 0.5, 10) <= 0.95:
            break
    assert 0.05 <= NC.mean2one_fraction(ps, pt, ls, lt, 0.5, 10) <= 0.95
    for meth in NC.SDA_METHODS:
        want = O.prob_weights_soft(ps, pt, ls, lt, 0.5, meth)
        got = NC.sda_weights(ps, pt, ls, lt, 0.5, meth, 10)
        assert got.shape == want.shape
        torch.testing.assert_close(got, want.double(), rtol=1e-4, atol=1e-9)
    D = 37
    X, Y = torch.randn(m, D, generator=g), torch.randn(m, D, generator=g) + 0.1
    w = torch.rand(1, m, generator=g) + 0.5
    for lsc in (5.0, 50.0):
        want = O.soft_mmd(ls, X, lt, Y, lsc, w)
        got = NC.soft_mmd(ls, X.double(), lt, Y.double(), lsc, w, 10)
        torch.testing.assert_close(got, want.double(), rtol=1e-4, atol=1e-6)
    same = NC.hard_mmd(ls, X.double(), ls.clone(), Y.double())
    torch.testing.assert_close(same, O.mix_rbf_mmd2(X, Y).double(), rtol=1e-4, atol=1e-6)


def test_restatement_cases_have_safe_mean2one_fractions():
    """Every SDA case of the GPU test: labels over the full range, and 1 / mean(distance) away from an integer."""
    for C in NC.SDA_COUNTS:
        for m in NC.SDA_ROWS:
            ps, pt, ls, lt = NC.sda_case(C, m)
            assert ps.shape == pt.shape == (m, C) and int(ls.max()) < C and int(ls.min()) >= 0
            assert 0.05 <= NC.mean2one_fraction(ps, pt, ls, lt, NC.LABEL_WEIGHT, C) <= 0.95
            if m == 300:
                assert int(torch.cat((ls, lt)).max()) == C - 1
