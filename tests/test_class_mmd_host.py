"""CPU: mmd.class_pairs_host, the plain-Python statement of the two row-pairing rules of the class-aligned MMD (the yardstick
of ops.class_pairs in tests/test_gpu_class_mmd.py), against torch.eq / get_most_overlapped_element."""
import pytest
import torch

from class_mmd_cases import label_sets

SETS = label_sets()
IDS = [s[0] for s in SETS]


@pytest.mark.parametrize('name,ls,lt,in_range', SETS, ids=IDS)
def test_hard_rule_is_the_equality_mask_in_index_order(name, ls, lt, in_range):
    from sug_amd.model import mmd
    ind_s, ind_t = mmd.class_pairs_host(ls, lt, 0)
    want = torch.eq(ls, lt).nonzero().reshape(-1).tolist()
    assert ind_s == want and ind_t == want


@pytest.mark.parametrize('num_class', [10, 40])
@pytest.mark.parametrize('name,ls,lt,in_range', SETS, ids=IDS)
def test_stable_rule_counts_members_and_order(name, ls, lt, in_range, num_class):
    from sug_amd.model import mmd
    ind_s, ind_t = mmd.class_pairs_host(ls, lt, 1, num_class)
    assert len(ind_s) == len(ind_t) and len(set(ind_s)) == len(ind_s) and len(set(ind_t)) == len(ind_t)
    pos = 0
    for c in range(num_class):
        rows_s, rows_t = (ls == c).nonzero().reshape(-1).tolist(), (lt == c).nonzero().reshape(-1).tolist()
        k = min(len(rows_s), len(rows_t))
        # the class's block: min(a_c, b_c) pairs, the lowest indices of the class on each side, ascending; classes ascending
        assert ind_s[pos:pos + k] == rows_s[:k] and ind_t[pos:pos + k] == rows_t[:k], (name, c)
        pos += k
    assert pos == len(ind_s)
    for lab, ind in ((ls, ind_s), (lt, ind_t)):                 # a label outside [0, num_class) is never selected
        assert all(0 <= int(lab[i]) < num_class for i in ind)
    assert [int(ls[i]) for i in ind_s] == [int(lt[i]) for i in ind_t]


@pytest.mark.parametrize('name,ls,lt,in_range', [s for s in SETS if s[3]], ids=[s[0] for s in SETS if s[3]])
def test_stable_rule_against_get_most_overlapped_element(name, ls, lt, in_range):
    """The same number of pairs per class as the reference's selection; the same index lists wherever torch.sort is stable
    (up to 16 elements), i.e. wherever the reference's choice of members is defined at all."""
    from sug_amd.model import mmd
    from sug_amd.utils.common_utils import get_most_overlapped_element
    ind_s, ind_t = mmd.class_pairs_host(ls, lt, 1)
    ref_s, ref_t = get_most_overlapped_element(ls, lt)
    assert len(ref_s) == len(ind_s)
    count = lambda lab, ind: torch.bincount(lab[torch.tensor(ind, dtype=torch.int64)], minlength=10).tolist()
    assert count(ls, ind_s) == count(ls, ref_s) == count(lt, ind_t) == count(lt, ref_t)
    if ls.numel() <= 16:
        assert ind_s == ref_s and ind_t == ref_t


def test_host_rule_rejects_an_unknown_mode_and_routes_nothing_on_the_cpu():
    """CPU tensors never reach the device path: hard_mmd keeps its composed lines there, 'stable' says what it needs."""
    from sug_amd import ops
    from sug_amd.model import mmd
    ls, lt = torch.tensor([0, 1]), torch.tensor([0, 2])
    with pytest.raises(RuntimeError):
        mmd.class_pairs_host(ls, lt, 2)
    X = torch.zeros(2, 4)
    assert not ops.class_mmd_supported(ls, X, lt, X)
    with pytest.raises(RuntimeError, match='stable'):
        mmd.max_hard_mmd(ls, X, lt, X, pairing='stable')
    with pytest.raises(RuntimeError, match='pairing'):
        mmd.max_hard_mmd(ls, X, lt, X, pairing='nope')
