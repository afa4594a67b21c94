"""Label sets shared by tests/test_class_mmd_host.py and tests/test_gpu_class_mmd.py (CPU tensors, made once, never written to)."""
import torch

RANDOM_M = (1, 5, 16, 17, 32, 80)


def random_labels(m, seed=None, hi=10):
    g = torch.Generator().manual_seed(1000 + m if seed is None else seed)
    return torch.randint(0, hi, (m,), generator=g), torch.randint(0, hi, (m,), generator=g)


def constructed():
    """name -> (label_s, label_t, in_range): every label of an in_range set lies in [0, 10)."""
    t = lambda v: torch.tensor(v, dtype=torch.int64)
    return {
        'same': (t([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]), t([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]), True),
        'one_match': (t([0, 1, 2, 3, 4]), t([5, 6, 7, 8, 4]), True),
        'disjoint': (t([0, 1, 2, 0, 1]), t([5, 6, 7, 8, 9]), True),
        # class 2 crowds the source, class 7 the target: which members are paired is the whole question
        'skewed': (t([2] * 11 + [7, 1, 2, 0]), t([7, 2, 7, 7, 2, 7, 0, 7, 2, 7, 7, 1, 7, 2, 7]), True),
        'permuted': (t([9, 8, 7, 6, 5, 4, 3, 2, 1, 0]), t([0, 1, 2, 3, 4, 5, 6, 7, 8, 9]), True),
        # labels outside [0, 10) on either side, some of them equal row by row (mode 0 pairs those, mode 1 never)
        'out_of_range': (t([0, 12, -1, 3, 3, 11, 12, 10]), t([12, 0, -1, 3, 7, 3, 12, 10]), False),
    }


def label_sets():
    """[(name, label_s, label_t, in_range)]: seeded random labels at RANDOM_M, then the constructed vectors."""
    out = [('rand%d' % m,) + random_labels(m) + (True,) for m in RANDOM_M]
    out += [(k,) + v for k, v in constructed().items()]
    return out


def mixed_labels(m):
    """Seeded random labels [m] with 0 < n < m under BOTH rules (the first draw of a fixed sequence that has it)."""
    from sug_amd.model import mmd
    for k in range(200):
        ls, lt = random_labels(m, seed=7000 + 131 * m + k)
        n0, n1 = len(mmd.class_pairs_host(ls, lt, 0)[0]), len(mmd.class_pairs_host(ls, lt, 1)[0])
        if 0 < n0 < m and 0 < n1 < m:
            return ls, lt
    raise AssertionError('no mixed label draw for m=%d' % m)
