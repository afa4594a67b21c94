"""Gaussian multi-kernel MMD alignment loss with SDA sample weights (mirror of the
reference's model/mmd.py: same function names, arguments and `args` dict keys).

The (2m x 2m) kernel-matrix reduction runs in one HIP kernel (sug_mmd_rbf); the SDA
weights are computed on the device (the reference round-trips them through the CPU,
model/mmd.py:138-142, :295).  The variance / ratio estimator and the linear-time estimators
(mix_rbf_mmd2_and_ratio, linear_mmd2, poly_mmd2) run in their own kernels (ops.mmd_ratio,
ops.linear_mmd2 / poly_mmd2), and so does the contrastive mode NAME: CL (contrastive_loss_weighted, ops.cl_loss)."""
from copy import deepcopy

import torch
import torch.nn as nn

from .. import ops
from ..chamfer_distance import ChamferDistance  # noqa: F401  (model/mmd.py:9 imports the third-party op under this name)
from ..utils.common_utils import create_one_hot_labels, get_most_overlapped_element

min_var_est = 1e-8
sigma_list = [0.01, 0.1, 1, 10, 100]


def _cl_criterion(args, CL_criterion=None):
    """The criterion of a NAME: CL term: the caller's, or the trainer's own construction (train_dg_single_gpu.py:236-242)
    with the margin of the term's MARGIN key."""
    if CL_criterion is not None:
        return CL_criterion
    return nn.CosineEmbeddingLoss(margin=float(args.get("MARGIN", 0.2)), reduction="none")


def mmd_cal(label_s, feat_s, label_t, feat_t, args: dict, data_s=None, data_t=None, KPC=False, sample_weights=None,
            CL_criterion=None):
    """model/mmd.py:25-41.  `sample_weights` (not in the reference signature): SDA weights the caller
    already has (the batch-sharded step computes them once from the gathered batch).  KPC=True (the KPConv
    backbone's call) uses the same Chamfer weights as KPC=False: the reference's KPC branch (model/mmd.py:122-124)
    only calls the unpinned third-party Chamfer op another way.  NAME: CL (not dispatched by the reference, whose trainer
    nevertheless builds its criterion) is contrastive_loss_weighted with `CL_criterion`, by default
    nn.CosineEmbeddingLoss(margin=args.get('MARGIN', 0.2), reduction='none').  The class count of the one-hot blocks,
    the class lists and the SDA weights is the term's args.get('NUM_CLASS', 10) (the reference hard-codes 10)."""
    num_class = int(args.get("NUM_CLASS", 10))
    sample_weights_flag = args.get("GEO_WEIGHTS", None) or args.get("SEM_WEIGHTS", None)
    if sample_weights is None and data_s is not None and sample_weights_flag:
        sample_weights = cal_sample_weights(data_s, data_t, args, label_s=label_s, label_t=label_t)
    if args["NAME"] == "SOFT_MMD":
        return soft_mmd(label_s, feat_s, label_t, feat_t, float(args["LABEL_SCALE"]), sample_weights=sample_weights,
                        num_class=num_class)
    elif args["NAME"] == "HARD_MMD":
        return hard_mmd(label_s, feat_s, label_t, feat_t, num_class=num_class)
    elif args["NAME"] == "MAX_HARD_MMD":
        return max_hard_mmd(label_s, feat_s, label_t, feat_t, pairing=args.get("PAIRING", "sorted"), num_class=num_class)
    elif args["NAME"] == "OFF":
        return mix_rbf_mmd2(feat_s, feat_t, sigma_list)
    elif args["NAME"] == "CL":
        return contrastive_loss_weighted(label_s, feat_s, label_t, feat_t, float(args.get("LABEL_SCALE", 0.0)),
                                         _cl_criterion(args, CL_criterion), sample_weights=sample_weights)
    raise RuntimeError("Not Supported MMD Method")


def cal_sample_weights(data_s, data_t, args, label_s=None, label_t=None, KPC=False, num_class=None):
    """model/mmd.py:44-53.  num_class: the class count of the SEM_WEIGHTS branch; None reads args.get('NUM_CLASS', 10)."""
    if num_class is None:
        num_class = int(args.get("NUM_CLASS", 10))
    if args.get("GEO_WEIGHTS", None):
        return geometric_weights(data_s, data_t, weighting=args["GEO_WEIGHTS"], KPC=KPC)
    elif args.get("ENTROPY_WEIGHTS", None):
        return entropy_weights(data_s, data_t, weighting=args["ENTROPY_WEIGHTS"])
    elif args.get("SEM_WEIGHTS", None):
        kw = {} if num_class == 10 else {"num_class": num_class}     # (the reference's count: the reference's own call)
        return prob_weights_soft(data_s, data_t, label_s, label_t, args["LABEL_WEIGHT"], args["SEM_WEIGHTS"], **kw)
    raise RuntimeError("Not suppprted weighting opperation")


def sda_weights_of(args, pred_s, pred_t, label_s, label_t, num_class=None):
    """The SDA weights of one semantic MMD term from (gathered) logits and labels, with mmd_cal's own rules: weights only
    if GEO_WEIGHTS or SEM_WEIGHTS is set (model/mmd.py:28), and then cal_sample_weights' precedence GEO > ENTROPY > SEM
    (:44-53).  The batch-sharded steps of SUGStep call this, so that every launch form weights a term the way
    mmd_cal(..., data_s=pred_s, data_t=pred_t) does.  num_class as in cal_sample_weights."""
    if not (args.get("GEO_WEIGHTS", None) or args.get("SEM_WEIGHTS", None)):
        return None
    return cal_sample_weights(pred_s, pred_t, args, label_s=label_s, label_t=label_t, num_class=num_class)


def soft_mmd(label_s, feat_s, label_t, feat_t, label_weight, sample_weights=None, num_class=10):
    """model/mmd.py:56-66: MMD on [features | one-hot(label, num_class) * label_weight]."""
    m = feat_s.shape[0]
    Z = ops.mmd_assemble(feat_s, feat_t, label_s, label_t, label_weight, num_class)    # [2m, D+C] = [feat | onehot * weight]
    return ops.mix_rbf_mmd2_rows(Z, m, sample_weights, sigma_list)


def soft_mmd_multi(label_s, label_t, terms, num_class=None):
    """[mmd_cal(label_s, feat_s, label_t, feat_t, args, data_s, data_t) for (feat_s, feat_t, args, data_s, data_t) in terms]
    for SOFT_MMD terms of one batch (model/mmd.py:25-41, :56-66; the three terms of train_dg_single_gpu.py:300-322): the
    SDA weights per term as mmd_cal forms them, then every stage of the terms in one launch (ops.soft_mmd_multi).
    num_class: the one class count of all terms; None reads the terms' NUM_CLASS keys (default 10), which must agree."""
    terms = list(terms)
    for _, _, args, _, _ in terms:
        if args["NAME"] != "SOFT_MMD":
            raise RuntimeError("soft_mmd_multi: SOFT_MMD terms only")
    num_class = _terms_num_class(terms, num_class, "soft_mmd_multi")
    ws = _terms_sample_weights(label_s, label_t, terms, num_class=num_class)
    packed = [(fs, ft, float(args["LABEL_SCALE"]), w) for (fs, ft, args, _, _), w in zip(terms, ws)]
    return ops.soft_mmd_multi(label_s, label_t, packed, sigma_list, num_class=num_class)


def _terms_num_class(terms, num_class, who):
    """The class count of a multi-term call: the caller's, or the terms' own NUM_CLASS (default 10), one for all."""
    if num_class is not None:
        return int(num_class)
    counts = {int(args.get("NUM_CLASS", 10)) for _, _, args, _, _ in terms}
    if len(counts) > 1:
        raise ValueError("%s: the terms of one call share one class count (NUM_CLASS: %s)" % (who, sorted(counts)))
    return counts.pop() if counts else 10


def _terms_sample_weights(label_s, label_t, terms, num_class=10):
    """The SDA weights of every (feat_s, feat_t, args, data_s, data_t) term of one batch as mmd_cal would form them (None
    for a term without), the terms weighted from head logits by one rule in one launch."""
    ws = [None] * len(terms)
    # terms weighted from head logits by the same rule (cal_sample_weights' third branch): their weights in one launch
    by_rule = {}
    for i, (_, _, args, data_s, data_t) in enumerate(terms):
        if data_s is None or not (args.get("GEO_WEIGHTS", None) or args.get("SEM_WEIGHTS", None)):
            continue
        if args.get("SEM_WEIGHTS", None) and not args.get("GEO_WEIGHTS", None) and not args.get("ENTROPY_WEIGHTS", None) \
                and data_s.is_cuda and data_s.shape[-1] == num_class and 2 <= num_class <= ops.SDA_MAX_CLASSES:
            by_rule.setdefault((float(args["LABEL_WEIGHT"]), args["SEM_WEIGHTS"]), []).append(i)
        else:
            ws[i] = cal_sample_weights(data_s, data_t, args, label_s=label_s, label_t=label_t, num_class=num_class)
    for (lw, rule), idx in by_rule.items():
        assert lw < 1, "For Entropy, Label weight should be less than one"
        outs = ops.sda_prob_weights_multi([(terms[i][3], terms[i][4]) for i in idx], label_s, label_t, lw, rule)
        for i, o in zip(idx, outs):
            ws[i] = o.reshape(1, -1)
    return ws


def cl_loss_multi(label_s, label_t, terms, num_class=None):
    """[mmd_cal(label_s, feat_s, label_t, feat_t, args, data_s, data_t) for (feat_s, feat_t, args, data_s, data_t) in terms]
    for NAME: CL terms of one batch, the sibling of soft_mmd_multi: the SDA weights per term as mmd_cal forms them, then
    all terms in one launch sequence (ops.cl_loss_multi) where ops.cl_loss_supported holds for every one of them, term by
    term through contrastive_loss_weighted otherwise.  num_class (the SDA weights' class count) as in soft_mmd_multi."""
    terms = list(terms)
    for _, _, args, _, _ in terms:
        if args["NAME"] != "CL":
            raise RuntimeError("cl_loss_multi: CL terms only")
    ws = _terms_sample_weights(label_s, label_t, terms, num_class=_terms_num_class(terms, num_class, "cl_loss_multi"))
    margins = [float(args.get("MARGIN", 0.2)) for _, _, args, _, _ in terms]
    if all(ops.cl_loss_supported(label_s, fs, label_t, ft, mg, w) for (fs, ft, _, _, _), mg, w in zip(terms, margins, ws)):
        return ops.cl_loss_multi(label_s, label_t, [(fs, ft, mg, w) for (fs, ft, _, _, _), mg, w in zip(terms, margins, ws)])
    return [contrastive_loss_weighted(label_s, fs, label_t, ft, float(args.get("LABEL_SCALE", 0.0)), _cl_criterion(args),
                                      sample_weights=w) for (fs, ft, args, _, _), w in zip(terms, ws)]


def soft_mmd_sharded(label_s, feat_s, label_t, feat_t, label_g, feat_g_s, label_tg, feat_g_t, label_weight, row0,
                     sample_weights=None, world=1, num_class=10):
    """soft_mmd of the GLOBAL batch from a rank's shard: feat_s / feat_t [mloc, D] are this
    rank's (differentiable) features, feat_g_s / feat_g_t [M, D] the gathered values of all ranks (this
    rank's rows at row0); equals soft_mmd(label_g, feat_g_s, label_tg, feat_g_t, ...) on every rank."""
    mloc, M = feat_s.shape[0], feat_g_s.shape[0]
    Zloc = ops.mmd_assemble(feat_s, feat_t, label_s, label_t, label_weight, num_class)
    Zall = ops.mmd_assemble(feat_g_s.detach(), feat_g_t.detach(), label_g, label_tg, label_weight, num_class)
    return ops.mix_rbf_mmd2_rows_sharded(Zloc, Zall, mloc, M, row0, sample_weights, sigma_list, world)


def hard_mmd(label_s, feat_s, label_t, feat_t, num_class=10):
    """model/mmd.py:69-77: MMD of the rows whose two labels agree.  On the device the rows are chosen there
    (ops.class_mmd, mode 0): no host wait, and a batch without such a row gives NaN with zero gradients as in the
    reference; otherwise (CPU tensors, beyond ops.class_mmd_supported's limits, SUG_CLASS_MMD=0) the composed lines.
    num_class only sizes the device kernel's class table: which rows agree does not depend on it."""
    if ops.class_mmd_supported(label_s, feat_s, label_t, feat_t, sigma_list, num_class=num_class):
        return ops.class_mmd(label_s, feat_s, label_t, feat_t, 0, sigma_list, num_class=num_class)
    same = torch.eq(label_s, label_t)
    return mix_rbf_mmd2(feat_s[same], feat_t[same], sigma_list)


def contrastive_loss_weighted(label_s, feat_s, label_t, feat_t, label_weight, CL_criterion, sample_weights=None):
    """model/mmd.py:80-94: the criterion's row-wise loss between paired rows, target +1 where the two labels agree and -1
    elsewhere, times the SDA weights, averaged over ALL rows.  `label_weight` takes no part: the reference builds the
    label-augmented features (:81-84) and then hands the plain ones to the criterion (:88); nothing is launched for them here.
    An nn.CosineEmbeddingLoss (exactly that class) with reduction 'none' on what ops.cl_loss_supported lists goes through
    ops.cl_loss with the criterion's margin; anything else (another callable, CPU tensors, fp64, SUG_CL_LOSS=0) through the
    composed lines."""
    if type(CL_criterion) is nn.CosineEmbeddingLoss and CL_criterion.reduction == 'none' \
            and ops.cl_loss_supported(label_s, feat_s, label_t, feat_t, CL_criterion.margin, sample_weights):
        return ops.cl_loss(label_s, feat_s, label_t, feat_t, CL_criterion.margin, sample_weights)
    same_class_index = 2 * torch.eq(label_s, label_t) - 1
    loss = CL_criterion(feat_s, feat_t, same_class_index)
    if sample_weights is not None:
        loss = torch.mul(sample_weights.squeeze().to(device=loss.device), loss)
    return torch.mean(loss)


def max_hard_mmd(label_s, feat_s, label_t, feat_t, pairing='sorted', num_class=10):
    """model/mmd.py:96-104.  pairing 'sorted' (the default) pairs the rows get_most_overlapped_element picks on the host:
    which members of an over-represented class those are follows from torch.sort's unstable order once m > 16.  pairing
    'stable' (args['PAIRING'] = 'stable') pairs the same NUMBER of rows per class but always the lowest indices
    (class_pairs_host, mode 1), chosen on the device (ops.class_mmd, mode 1: no host wait, capturable); it needs what
    ops.class_mmd_supported states.  Labels outside [0, num_class) are never paired there and raise nothing."""
    if pairing == 'stable':
        if not ops.class_mmd_supported(label_s, feat_s, label_t, feat_t, sigma_list, num_class=num_class):
            raise RuntimeError("max_hard_mmd(pairing='stable') runs on the HIP device within ops.class_mmd_supported's limits "
                               "(and not with SUG_CLASS_MMD=0)")
        return ops.class_mmd(label_s, feat_s, label_t, feat_t, 1, sigma_list, num_class=num_class)
    if pairing != 'sorted':
        raise RuntimeError("max_hard_mmd: pairing 'sorted' or 'stable' (got %r)" % (pairing,))
    ind_s, ind_t = get_most_overlapped_element(label_s.cpu(), label_t.cpu(), num_class=num_class)
    assert len(ind_s) == len(ind_t), "The feature shape mis-matched"
    return mix_rbf_mmd2(feat_s[ind_s], feat_t[ind_t], sigma_list)


def class_pairs_host(label_s, label_t, mode, num_class=10):
    """The rows a class-aligned MMD pairs, as two Python index lists (ind_s, ind_t) from CPU label tensors: the rule that
    ops.class_pairs implements on the device, restated plainly.
      mode 0 (hard_mmd): every i with label_s[i] == label_t[i], ascending; ind_s == ind_t.
      mode 1 (max_hard_mmd, pairing 'stable'): for c = 0 .. num_class-1 in order, the first min(a_c, b_c) rows of class c of
      the source paired with the first min(a_c, b_c) rows of class c of the target, lowest index first.  Labels outside
      [0, num_class) are never paired."""
    ls, lt = [int(v) for v in label_s.reshape(-1).tolist()], [int(v) for v in label_t.reshape(-1).tolist()]
    assert len(ls) == len(lt)
    if mode == 0:
        ind = [i for i in range(len(ls)) if ls[i] == lt[i]]
        return ind, list(ind)
    if mode != 1:
        raise RuntimeError('class_pairs_host: mode 0 (hard) or 1 (stable max-overlap)')
    ind_s, ind_t = [], []
    for c in range(num_class):
        rows_s = [i for i, v in enumerate(ls) if v == c]
        rows_t = [i for i, v in enumerate(lt) if v == c]
        k = min(len(rows_s), len(rows_t))
        ind_s += rows_s[:k]
        ind_t += rows_t[:k]
    return ind_s, ind_t


def chamfer_distances(pc_s, pc_t):
    """Per-pair Chamfer distance [m] of paired clouds ([m,3,N(,1)] or [m,N,3]): cd_distance,
    model/mmd.py:169-175 (mean of dist1 + mean of dist2)."""
    return ops.chamfer(*_chamfer_rows(pc_s, pc_t))


def cd_distance(pc1, pc2, chamfer_dist, batch_loss=True):
    """model/mmd.py:169-175: the Chamfer loss of paired clouds pc1 [B,N,3], pc2 [B,M,3] through the op `chamfer_dist` (a
    ChamferDistance()): per pair [B] (batch_loss=True) or the scalar mean(dist1) + mean(dist2).  Differentiable with respect
    to both clouds in both forms (geometric_weights and chamfer_distances keep their detached one-launch path)."""
    dist1, dist2, idx1, idx2 = chamfer_dist(pc1, pc2)
    if not batch_loss:
        loss = (torch.mean(dist1)) + (torch.mean(dist2))
    else:
        loss = torch.mean(dist1, dim=1) + torch.mean(dist2, dim=1)
    return loss


def _chamfer_rows(pc_s, pc_t):
    assert pc_s.shape[0] == pc_t.shape[0]
    # the reference's own layout test (model/mmd.py:110): channel-first when dim 1 has 3 entries.  [m,N,3] rows with N == 3
    # are therefore read as channel-first, exactly as there; internal callers only pass rows when N != 3
    if pc_s.shape[1] == 3:
        a = pc_s.reshape(pc_s.shape[0], 3, -1).transpose(1, 2)
        b = pc_t.reshape(pc_t.shape[0], 3, -1).transpose(1, 2)
    else:
        a, b = pc_s, pc_t
    return a, b


def geometric_weights(pc_s, pc_t, metric="chamfer_distance", weighting="none", KPC=False):
    """model/mmd.py:107-131: Chamfer distance between paired clouds -> weights [1,m].
    The reference calls a third-party ChamferDistance op; sug_chamfer follows its call-site
    contract (parity unpinned, see oracle/ref_cpu.py:chamfer_weights)."""
    if metric != "chamfer_distance":
        raise RuntimeError("Currently Only Support CD distance")
    if weighting in ("naive_inverse", "exp_inverse", "mean2one") and pc_s.is_cuda:
        a, b = _chamfer_rows(pc_s, pc_t)
        return ops.chamfer_weights(a, b, weighting).reshape(1, -1)      # the weighting in the distance's own fold launch
    distance = chamfer_distances(pc_s, pc_t)
    return distance2weights(distances=distance, method=weighting).reshape(1, -1)


def normalized(vec):
    """model/mmd.py:151-153 (global-sum normalisation)."""
    vec = vec + min_var_est
    return vec / torch.sum(vec)


def _kl_div(x, y):
    """scipy.special.kl_div (dataset_splitter.py:244-245 uses it both ways), all three branches: x log(x/y) - x + y for
    x, y > 0; y for x == 0, y >= 0; +inf otherwise.  A saturated softmax row has an fp32 entropy of exactly -0.0: the
    reference then reports an infinite distance for that pair, where the plain formula gives NaN (golden
    entropy.npz, keys ps1 / w1_*)."""
    inf = torch.full_like(x, float('inf'))
    main = x * torch.log(x / y) - x + y
    out = torch.where((x > 0) & (y > 0), main, torch.where((x == 0) & (y >= 0), y, inf))
    return torch.where(torch.isnan(x) | torch.isnan(y), x + y, out)           # (NaN in, NaN out -- scipy's first branch)


def cal_probs2entropy(probs):
    """dataset_splitter.py:234-241: -(p log(p + 1e-30)).sum(1) of the rows of probs [m, C]."""
    return -(probs * torch.log(probs + 1e-30)).sum(1)


def entropy_dis(pred_s, pred_t):
    """model/mmd.py:161-166: symmetric KL (dataset_splitter.py:244-245, scipy kl_div element-wise) between the
    prediction entropies of paired source / target samples -> [m]."""
    es, et = cal_probs2entropy(pred_s.detach()), cal_probs2entropy(pred_t.detach())
    return _kl_div(es, et) * 0.5 + _kl_div(et, es) * 0.5


def entropy_weights(pred_s, pred_t, weighting="exp_inverse"):
    """model/mmd.py:155-158, on the device (the reference returns a CPU tensor): [1, m] weights from entropy_dis.  As in the
    reference the inputs must be PROBABILITIES (logits put a negative number under the log: NaN there and here); the
    reference itself runs only for weighting 'none' / 'mean2one' -- its 'exp_inverse' / 'naive_inverse' build Python lists
    that distance2weights then fails to reshape; here they follow their evident formulas -- and 'hist' raises in both."""
    return distance2weights(distances=entropy_dis(pred_s, pred_t), method=weighting).reshape(1, -1)


def prob_weights_soft(pred_s, pred_t, label_s, label_t, label_weight, weighting="mean2one", num_class=10):
    """model/mmd.py:134-148, on the device.  num_class (10 in the reference) is the width of the logits: a mismatch is a
    ValueError.  HIP tensors of 2 to ops.SDA_MAX_CLASSES (64) classes go through one kernel; CPU tensors and wider logits
    through the composed lines below with the same count.  In the kernel a label outside [0, num_class) gets no one-hot
    entry and raises nothing (the composed lines scatter with it and fail as torch does)."""
    assert label_weight < 1, "For Entropy, Label weight should be less than one"
    num_class = int(num_class)
    if pred_s.shape[-1] != num_class or pred_t.shape[-1] != num_class:
        raise ValueError("prob_weights_soft: the logits are %d / %d wide but num_class is %d"
                         % (pred_s.shape[-1], pred_t.shape[-1], num_class))
    if pred_s.is_cuda and 2 <= num_class <= ops.SDA_MAX_CLASSES:        # one kernel instead of ~40 tiny ones
        return ops.sda_prob_weights(pred_s, pred_t, label_s, label_t, label_weight, weighting).reshape(1, -1)
    a = torch.cat((torch.softmax(pred_s.detach(), dim=1).view(-1, num_class),
                   create_one_hot_labels(label_s, num_class) * label_weight), dim=1)
    b = torch.cat((torch.softmax(pred_t.detach(), dim=1).view(-1, num_class),
                   create_one_hot_labels(label_t, num_class) * label_weight), dim=1)
    a, b = normalized(a), normalized(b)
    distance = (_kl_div(a, b) * 0.5 + _kl_div(b, a) * 0.5).sum(1)
    return distance2weights(distances=distance, method=weighting).reshape(1, -1)


def distance2weights(distances, method="naive_inverse"):
    """model/mmd.py:178-202 for tensor inputs ('mean2one' truncates 1/mean to an integer, :200)."""
    if method == "naive_inverse":
        w = 1 / (distances + min_var_est)
        weights = w / w.sum()
    elif method == "exp_inverse":
        w = torch.exp(-distances)
        weights = w / w.sum()
    elif method == "none":
        weights = deepcopy(distances)
    elif method == "mean2one":
        scale_ = (1 / distances.mean()).type(torch.int)
        weights = distances * scale_
    elif method == "hist":
        # model/mmd.py:186-193 assigns into a Python list with a tuple of index arrays: a TypeError in the reference on
        # every input; there is no behaviour to mirror
        raise TypeError("distance2weights('hist'): list indices must be integers or slices, not tuple "
                        "(the reference's own failure, model/mmd.py:193)")
    else:
        raise RuntimeError("Not supported weighting method %s" % method)
    return weights.reshape(-1, 1).squeeze()


def mix_rbf_mmd2(X, Y, sigma_list, biased=True, sample_weights=None):
    """model/mmd.py:257-260 with _mmd2, :274-312: biased (the estimator every caller of the reference uses) or unbiased."""
    assert X.size(0) == Y.size(0)
    return ops.mix_rbf_mmd2_rows(torch.cat((X, Y), 0), X.size(0), sample_weights, sigma_list, biased=biased)


def linear_mmd2(f_of_X, f_of_Y):
    """model/mmd.py:211-216: the linear-time estimator with the linear kernel, the mean over adjacent rows of
    <x_i - y_i, x_{i+1} - y_{i+1}>.  fp32 HIP tensors with at least two rows go through ops.linear_mmd2; anything else
    (CPU tensors, other dtypes, one row: the mean of nothing, NaN as in the reference) through the composed lines."""
    if ops.adjacent_mmd_supported(f_of_X, f_of_Y):
        return ops.linear_mmd2(f_of_X, f_of_Y)
    delta = f_of_X - f_of_Y
    return torch.mean((delta[:-1] * delta[1:]).sum(1))


def poly_mmd2(f_of_X, f_of_Y, d=2, alpha=1.0, c=2.0):
    """model/mmd.py:223-236: the linear-time estimator with the kernel (alpha <x, y> + c)^d over adjacent rows.  An integer
    d in 1..8 on fp32 HIP tensors goes through ops.poly_mmd2; a non-integer or larger d and everything linear_mmd2 lists
    through the composed lines."""
    if ops.adjacent_mmd_supported(f_of_X, f_of_Y, d):
        return ops.poly_mmd2(f_of_X, f_of_Y, d, alpha, c)

    def mean_k(A, B):
        return torch.mean((alpha * (A[:-1] * B[1:]).sum(1) + c).pow(d))

    return mean_k(f_of_X, f_of_X) + mean_k(f_of_Y, f_of_Y) - mean_k(f_of_X, f_of_Y) - mean_k(f_of_Y, f_of_X)


def mix_rbf_mmd2_and_ratio(X, Y, sigma_list, biased=True):
    """model/mmd.py:263-266 with _mmd2_and_ratio / _mmd2_and_variance (const_diagonal=False), :315-373: (loss, mmd2, var_est)
    with loss = mmd2 / sqrt(max(var_est, 1e-8)), the t-statistic objective.  fp32 HIP tensors within
    ops.mmd_ratio_supported's limits go through ops.mmd_ratio; anything else (CPU tensors, other dtypes, and m = 1, where
    the reference divides by m - 1 = 0 in Python and raises ZeroDivisionError, as these lines do) through the composed lines
    _mix_rbf_kernel / _mmd2_and_variance below."""
    assert X.size(0) == Y.size(0)
    m = X.size(0)
    if ops.mmd_ratio_supported(X, Y, sigma_list):
        return ops.mmd_ratio(torch.cat((X, Y), 0), m, sigma_list, biased=biased)
    mmd2, var_est = _mmd2_and_variance(*_mix_rbf_kernel(X, Y, sigma_list), biased=biased)
    return mmd2 / torch.sqrt(torch.clamp(var_est, min=min_var_est)), mmd2, var_est


def _mix_rbf_kernel(X, Y, sigma_list):
    """model/mmd.py:239-254: the blocks K_XX, K_XY, K_YY of the Gaussian multi-kernel matrix of [X ; Y], composed."""
    m = X.size(0)
    Z = torch.cat((X, Y), 0)
    ZZT = torch.mm(Z, Z.t())
    n = torch.diag(ZZT).unsqueeze(1).expand_as(ZZT)
    e = n - 2 * ZZT + n.t()
    K = 0.0
    for sigma in sigma_list:
        K = K + torch.exp(-(1.0 / (2 * sigma ** 2)) * e)
    return K[:m, :m], K[:m, m:], K[m:, m:]


def _mmd2_and_variance(K_XX, K_XY, K_YY, biased=False):
    """model/mmd.py:321-373 with const_diagonal=False: (mmd2, var_est) from the three blocks, composed."""
    m = K_XX.size(0)
    dX, dY = torch.diag(K_XX), torch.diag(K_YY)
    a, b = K_XX.sum(dim=1) - dX, K_YY.sum(dim=1) - dY           # Kt_XX e, Kt_YY e (Kt: without the diagonal)
    c, r = K_XY.sum(dim=0), K_XY.sum(dim=1)                     # K_XY^T e, K_XY e
    A, B, C = a.sum(), b.sum(), c.sum()
    FXX, FYY, FXY = (K_XX ** 2).sum() - dX.dot(dX), (K_YY ** 2).sum() - dY.dot(dY), (K_XY ** 2).sum()
    if biased:
        mmd2 = (A + dX.sum()) / (m * m) + (B + dY.sum()) / (m * m) - 2.0 * C / (m * m)
    else:
        mmd2 = A / (m * (m - 1)) + B / (m * (m - 1)) - 2.0 * C / (m * m)
    var_est = (2.0 / (m ** 2 * (m - 1.0) ** 2) * (2 * a.dot(a) - FXX + 2 * b.dot(b) - FYY)
               - (4.0 * m - 6.0) / (m ** 3 * (m - 1.0) ** 3) * (A ** 2 + B ** 2)
               + 4.0 * (m - 2.0) / (m ** 3 * (m - 1.0) ** 2) * (r.dot(r) + c.dot(c))
               - 4.0 * (m - 3.0) / (m ** 3 * (m - 1.0) ** 2) * FXY
               - (8 * m - 12) / (m ** 5 * (m - 1)) * C ** 2
               + 8.0 / (m ** 3 * (m - 1.0)) * (1.0 / m * (A + B) * C - a.dot(r) - b.dot(c)))
    return mmd2, var_est
