"""What tests/test_num_class_host.py and tests/test_gpu_num_class.py share: an fp64 restatement of the reference's
class-count-dependent lines for ANY class count C, and the inputs of the cases (CPU tensors, made once, never written to).

The reference itself runs ten classes only (model/mmd.py hard-codes `.view(-1, 10)` and `num_class=10`), and so does
oracle/ref_cpu.py, so the expected values at other counts are these lines:
    soft_mmd               model/mmd.py:56-66    MMD on [features | one-hot(label, C) * label_scale]
    prob_weights_soft      model/mmd.py:134-148  a = normalized([softmax(pred) | one-hot(label, C) * label_weight]), b likewise,
                                                 distance_i = sum_c 0.5 kl(a, b) + 0.5 kl(b, a), kl(x, y) = x log(x / y) - x + y
    distance2weights       model/mmd.py:178-202  none | naive_inverse | exp_inverse | mean2one (1 / mean truncated to an integer)
with the 10 replaced by C and evaluated in the dtype asked for (fp64 for the expected values; fp32 to measure what plain
fp32 arithmetic of the same lines loses).  tests/test_num_class_host.py pins them at C = 10 against the oracle before they
are trusted anywhere else.

Run as a script (`python tests/num_class_cases.py RESULTS.json`) this file holds the eval_worker case of
tests/test_gpu_num_class.py, which needs a process of its own for the reason tests/eval_worker_cases.py states."""
import functools
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import ref_cpu as O  # noqa: E402

EPS = 1e-8                                         # min_var_est, model/mmd.py:17
SDA_COUNTS = (2, 9, 11, 32, 40, 64)
SDA_ROWS = (5, 300)
SDA_METHODS = ('none', 'naive_inverse', 'exp_inverse', 'mean2one')
SDA_TOL = dict(rtol=2e-4, atol=1e-7)               # the project's tolerance for this kernel (tests/test_gpu_mmd.py:93)
LABEL_WEIGHT = 0.5


# ------------------------------------------------------------------------------------------------ the restatement
def one_hot(labels, C, dtype=torch.float64):
    """create_one_hot_labels (utils/common_utils.py:161-164) for C classes."""
    oh = torch.zeros(labels.shape[0], C, dtype=dtype)
    oh[torch.arange(labels.shape[0]), labels] = 1
    return oh


def sda_distances(ps, pt, ls, lt, label_weight, C, dtype=torch.float64):
    """model/mmd.py:134-148 up to the distances [m]."""
    assert ps.shape[1] == pt.shape[1] == C

    def aug(pred, lab):
        v = torch.cat((torch.softmax(pred.to(dtype), dim=1).view(-1, C), one_hot(lab, C, dtype) * label_weight), dim=1) + EPS
        return v / v.sum()

    def kl(x, y):
        return x * torch.log(x / y) - x + y
    a, b = aug(ps, ls), aug(pt, lt)
    return (kl(a, b) * 0.5 + kl(b, a) * 0.5).sum(1)


def distance2weights(d, method):
    """model/mmd.py:178-202."""
    if method == 'none':
        return d.clone()
    if method == 'naive_inverse':
        w = 1 / (d + EPS)
        return w / w.sum()
    if method == 'exp_inverse':
        w = torch.exp(-d)
        return w / w.sum()
    if method == 'mean2one':
        return d * (1 / d.mean()).type(torch.int)
    raise ValueError(method)


def sda_weights(ps, pt, ls, lt, label_weight, method, C, dtype=torch.float64):
    """prob_weights_soft for C classes -> [1, m]."""
    return distance2weights(sda_distances(ps, pt, ls, lt, label_weight, C, dtype), method).reshape(1, -1)


def mean2one_fraction(ps, pt, ls, lt, label_weight, C):
    """The fractional part of 1 / mean(distance) in fp64: 'mean2one' truncates that number, so a case whose fraction is
    near 0 or 1 would test the last bits of the mean, not the kernel."""
    r = float(1 / sda_distances(ps, pt, ls, lt, label_weight, C).mean())
    return r - int(r)


def soft_mmd(ls, X, lt, Y, label_scale, w, C):
    """model/mmd.py:56-66 in the dtype of X (the oracle's kernel-matrix lines are dtype-agnostic)."""
    Xa = torch.cat((X, one_hot(ls, C, X.dtype) * label_scale), dim=1)
    Ya = torch.cat((Y, one_hot(lt, C, Y.dtype) * label_scale), dim=1)
    return O.mix_rbf_mmd2(Xa, Ya, O.SIGMAS, None if w is None else w.to(X.dtype))


def hard_mmd(ls, X, lt, Y):
    """model/mmd.py:69-77."""
    same = torch.eq(ls, lt)
    return O.mix_rbf_mmd2(X[same], Y[same])


def max_hard_mmd_stable(ls, X, lt, Y, C):
    """model/mmd.py:96-104 with the 'stable' pairing: per class c < C the first min(a_c, b_c) rows of either side."""
    ind_s, ind_t = [], []
    for c in range(C):
        rs, rt = (ls == c).nonzero().flatten().tolist(), (lt == c).nonzero().flatten().tolist()
        k = min(len(rs), len(rt))
        ind_s += rs[:k]
        ind_t += rt[:k]
    return O.mix_rbf_mmd2(X[ind_s], Y[ind_t])


def cross_entropy(logits, label):
    return torch.nn.functional.cross_entropy(logits, label)


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def sda_case(C, m):
    """(ps, pt, ls, lt) for C classes and m rows, labels over the full range: the first seed (counted up from 1000 C + m)
    whose fp64 fraction of 1 / mean lies in [0.05, 0.95]."""
    for seed in range(1000 * C + m, 1000 * C + m + 200):
        g = torch.Generator().manual_seed(seed)
        ps, pt = torch.randn(m, C, generator=g) * 2, torch.randn(m, C, generator=g) * 2
        ls, lt = torch.randint(0, C, (m,), generator=g), torch.randint(0, C, (m,), generator=g)
        if 0.05 <= mean2one_fraction(ps, pt, ls, lt, LABEL_WEIGHT, C) <= 0.95:
            return ps, pt, ls, lt
    raise AssertionError('no seed with a safe mean2one fraction for C=%d m=%d' % (C, m))


@functools.lru_cache(maxsize=None)
def sda_expected(C, m, method):
    return sda_weights(*sda_case(C, m), LABEL_WEIGHT, method, C)


@functools.lru_cache(maxsize=None)
def mmd_case(C=11, m=8, D=266):
    """Features, labels over the full range (the last class present; three rows whose labels agree, classes present on one
    side only) and sample weights for the MMD terms."""
    g = torch.Generator().manual_seed(100 * C + m)
    X, Y = torch.randn(m, D, generator=g), torch.randn(m, D, generator=g) + 0.1
    ls = torch.tensor([C - 1, 0, 3, C - 1, 5, 7, 3, 1])[:m]
    lt = torch.tensor([C - 1, 3, 3, 2, C - 1, 7, 0, C - 2])[:m]
    w = torch.rand(1, m, generator=g) + 0.5
    return X, Y, ls, lt, w


def step_labels(C, B=4):
    """Four label pairs per step batch, drawn over the full range with the last class present."""
    g = torch.Generator().manual_seed(C)
    out = []
    for _ in range(3):
        ls, lt = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
        ls[0], lt[1] = C - 1, C - 1
        out.append((ls, lt))
    return out


# ------------------------------------------------------------------------------------------------ the eval_worker case
def case_eval_worker_eleven_classes():
    """eval_worker with num_class = 11 on two batches of an 11-class Net_MDA against the restated eager loop, as
    tests/eval_worker_cases.py compares (metrics bit for bit, loss within 1e-6)."""
    import copy
    import logging
    import torch.nn as nn
    import eval_worker_cases as E
    from sug_amd.model.Model import Net_MDA
    from sug_amd.utils.eval_utils import LAST, eval_worker
    C, B, N = 11, 8, 1024
    net = Net_MDA('Pointnet', num_class=C)
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 3))
    net = net.cuda().train()
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    with torch.no_grad():
        net(O.synth_clouds(B, N, g).cuda())                                     # BatchNorm running buffers
    net.eval()
    batches = []
    for b in (B, B // 2):
        lab = torch.randint(0, C, (b,), generator=g)
        lab[0] = C - 1                                                          # the class beyond the reference's ten
        batches.append((O.synth_clouds(b, N, g).cuda(), lab.cuda()))
    ce = nn.CrossEntropyLoss().cuda()
    torch.manual_seed(11)
    with torch.no_grad():
        ref = E.restated_loop(copy.deepcopy(net), batches, ce, C, False, True)
    torch.manual_seed(11)
    with torch.no_grad():
        res = eval_worker(E._eval_dict(copy.deepcopy(net), batches, ce, num_class=C), logging.getLogger('num_class_cases'))
    E._compare(res, ref)
    assert LAST['form'] == 'device' and LAST['class_acc'].shape == (C, 3)
    assert ref['class_acc'][C - 1, 1] == 2                                      # class 10 was scored in both batches


def main(out_path):
    from sug_amd.model.Model import Net_MDA
    Net_MDA.call_graphs = False             # the form tests/conftest.py pins for every test
    res = {}
    try:
        case_eval_worker_eleven_classes()
        res['eval_worker_eleven_classes'] = None
    except Exception:
        res['eval_worker_eleven_classes'] = traceback.format_exc()
    with open(out_path, 'w') as fh:
        json.dump(res, fh)


if __name__ == '__main__':
    main(sys.argv[1])
