"""dataset_splitter.py on the device: the geometric and the entropy sub-domain split of ONE dataset, on resident tensors.

The reference tool reads `.npy` files, registers every cloud of a class against an anchor with one open3d call per cloud
and writes one `.npy` per (class, cluster), which train_files_spliter.include_dataset_from_splitter later globs and
concatenates.  Here the dataset is a device tensor [M, P, 3], one anchor try is ONE launch of sug_icp_fitness over all
clouds of the class, and as_dataset_spliter() returns the dictionary create_splitted_dataset hands to UnifiedPointDG.
The k-means split (t-SNE) and the file layout are not mirrored.  Everything refuses CPU tensors.

    split = split_dataset_geometric(pts, labels, generator=np.random.default_rng(0))
    parts = as_dataset_spliter(pts, labels, split)
    sets = [UnifiedPointDG(kind, parts[k]['pts'], parts[k]['label'], ...) for k in ('subset_1', 'subset_2')]
"""
import collections
import warnings

import numpy as np
import torch

from . import ops
from .data import data_utils
from .model.mmd import cal_probs2entropy

MAX_TRIES = 5                    # anchor draws per class (dataset_splitter.py:76)
MAX_CORR_DIST = 0.15             # icp_distance's max_correspondence_distance (:230)
PFH_DIV, PFH_NNEIGHBORS, PFH_RAD = 2, 8, 0.2     # metric='pfh': get_pfh_descriptor's PFH(0.1, 2, 8, 0.2) (utils/pfh.py:117)

GeometricSplit = collections.namedtuple('GeometricSplit', 'indices cluster_labels distances anchors tries')
GeometricSplit.__doc__ = """Per class (lists of num_class entries): `indices` int64 [n] = the class's clouds in the order of
their smallest raw x, `cluster_labels` int64 [n] in {0, 1} and `distances` fp64 [n] (1 - fitness to the kept anchor), all
device tensors in that order; `anchors` (position of the kept anchor in the sorted order) and `tries` are host ints."""


def _clouds(pts, what):
    ops._need_gpu(pts)
    if pts.dim() != 3 or pts.shape[2] < 3:
        raise ValueError('%s: expected clouds [M, P, C>=3], got %s' % (what, tuple(pts.shape)))
    return pts[:, :, :3].to(torch.float32).contiguous()


def process_pts(pts, pt_num=500, return_index=False):
    """fps(normal_pc(cloud), pt_num) of dataset_splitter.py:48 for M clouds at once: pts [M, P, 3] -> [M, pt_num, 3] fp32,
    farthest-point sampling from point 0 (data/data_utils.py:185-229 starts there; ties -> lowest index, as its argmax over
    the ascending remaining points).  return_index: also the chosen point indices int32 [M, pt_num]."""
    x = _clouds(pts, 'process_pts')
    M, P, _ = x.shape
    if not 1 <= pt_num <= P:
        raise ValueError('process_pts: pt_num=%d of %d points per cloud' % (pt_num, P))
    x = data_utils.normal_pc(x).contiguous()
    idx = ops.fps(x, int(pt_num), torch.zeros(M, dtype=torch.int32, device=x.device))
    out = torch.gather(x, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
    return (out, idx) if return_index else out


def icp_distance(pts1, pts2):
    """1 - fitness of registration_icp(source=pts1, target=pts2, max_correspondence_distance=0.15)
    (dataset_splitter.py:217-231): pts1 [n1, 3]; pts2 [n2, 3] -> a 0-dim fp64 device tensor, or [M, n2, 3] -> [M] in one
    launch."""
    ops._need_gpu(pts1, pts2)
    single = pts2.dim() == 2
    tgt = (pts2.unsqueeze(0) if single else pts2)[..., :3].to(torch.float32)
    src = pts1[..., :3].to(torch.float32)
    count = ops.icp_fitness(src, tgt, max_corr_dist=MAX_CORR_DIST)[0]
    d = 1.0 - count.to(torch.float64) / float(src.shape[-2])
    return d[0] if single else d


def _geometric_labels(distances, use_hist=False):
    """The cut of dataset_splitter.py:62-69 on a host array of distances: label 0 below the mean (or below the middle edge
    of a 2-bin histogram), else 1; accepted when |n0 - 0.5 n| < 0.4 n.  -> (labels int64 [n], accepted)."""
    d = np.asarray(distances, dtype=np.float64)
    n = d.shape[0]
    threshold = np.histogram(d, bins=2)[1][1] if use_hist else np.mean(d)
    below = d < threshold
    labels = np.ones(n, dtype=np.int64)
    labels[below] = 0
    return labels, bool(np.abs(int(below.sum()) - 0.5 * n) < 0.4 * n)


def _split_class(n, distance_of, draw, use_hist=False, what='class'):
    """The anchor loop of dataset_splitter.py:56-79 for a class of n clouds: draw() -> an anchor position, distance_of(anchor)
    -> the n distances (host array); at most MAX_TRIES tries, the last one is kept with a warning.
    -> (labels, distances, anchor, tries)."""
    for tries in range(1, MAX_TRIES + 1):
        anchor = int(draw())
        if not 0 <= anchor < n:
            raise ValueError('%s: anchor %d outside the %d clouds' % (what, anchor, n))
        d = np.asarray(distance_of(anchor), dtype=np.float64)
        labels, accepted = _geometric_labels(d, use_hist)
        if accepted:
            break
    else:
        warnings.warn('%s: cannot find a suitable split in %d tries, keeping the last one' % (what, MAX_TRIES))
    return labels, d, anchor, tries


def _pfh_distance_of(processed):
    """metric='pfh': the descriptors of a class's processed clouds, computed once -> distance_of(anchor), ONE
    sug_pfh_hist_distance launch of the anchor's histograms against all of them (utils/pfh.py's pfh_hist_distance)."""
    hist, _, _, cnt, _ = ops.pfh_descriptors(processed, PFH_RAD, PFH_NNEIGHBORS, PFH_DIV)

    def distance_of(anchor):
        d = ops.pfh_hist_distance(hist[anchor], cnt[anchor], hist, cnt).cpu().numpy()
        if np.isnan(d).any():
            raise ValueError('split_dataset_geometric: metric=\'pfh\': cloud(s) %s of the class have no point with a neighbour '
                             'inside %g, so no histogram distance' % (np.flatnonzero(np.isnan(d)).tolist()[:8], PFH_RAD))
        return d
    return distance_of


def split_dataset_geometric(pts, labels, cluster_num=2, use_hist=False, num_class=10, generator=None, anchors=None,
                            pt_num=500, metric='icp'):
    """split_dataset_geometric of dataset_splitter.py:32-84 on a resident dataset: pts [M, P, 3] device tensor, labels [M]
    (host or device).  Per class: stable sort by the smallest raw x, process_pts, an anchor drawn from
    arange(n // 4, n // 2) of that order with `generator` (a numpy.random.Generator; default: a fresh default_rng()) or
    taken from anchors[cls] (up to five positions, used in order), the distances of all clouds to it in one launch, and the
    cut of _geometric_labels().  One host read of the n distances per try.  metric: 'icp' (the reference's, 1 - fitness) or
    'pfh' (the histogram distance of utils/pfh.py between the anchor's and every cloud's Point Feature Histograms, the
    descriptors computed once per class).  -> GeometricSplit."""
    if metric not in ('icp', 'pfh'):
        raise ValueError('split_dataset_geometric: metric=%r: \'icp\' or \'pfh\'' % (metric,))
    if cluster_num != 2:
        raise ValueError('Geometric Split Only Support 2 clusters (cluster_num=%r)' % (cluster_num,))
    lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1)
    if lab.shape[0] != pts.shape[0]:
        raise ValueError('split_dataset_geometric: %d labels for %d clouds' % (lab.shape[0], pts.shape[0]))
    per_class = [np.flatnonzero(lab == cls) for cls in range(num_class)]
    for cls, members in enumerate(per_class):
        if members.shape[0] < 4:
            raise ValueError('split_dataset_geometric: class %d has %d clouds, the anchor range arange(n // 4, n // 2) '
                             'needs at least 4' % (cls, members.shape[0]))
    x = _clouds(pts, 'split_dataset_geometric')
    if generator is None and anchors is None:
        generator = np.random.default_rng()
    out = GeometricSplit([], [], [], [], [])
    for cls, members in enumerate(per_class):
        n = members.shape[0]
        members = torch.as_tensor(members, dtype=torch.int64).to(x.device)
        raw = x.index_select(0, members)
        order = torch.sort(raw[:, :, 0].amin(dim=1), stable=True)[1]
        processed = process_pts(raw.index_select(0, order), pt_num)

        given = iter(anchors[cls]) if anchors is not None else None

        def draw():
            if given is None:
                return generator.choice(np.arange(n // 4, n // 2))
            try:
                return next(given)
            except StopIteration:
                raise ValueError('split_dataset_geometric: anchors[%d] ran out before a try was accepted' % cls) from None

        distance_of = (_pfh_distance_of(processed) if metric == 'pfh'
                       else lambda a: icp_distance(processed[a], processed).cpu().numpy())
        labels_c, d, anchor, tries = _split_class(n, distance_of, draw, use_hist, 'class %d' % cls)
        out.indices.append(members.index_select(0, order))
        out.cluster_labels.append(torch.as_tensor(labels_c).to(x.device))
        out.distances.append(torch.as_tensor(d).to(x.device))
        out.anchors.append(anchor)
        out.tries.append(tries)
    return out


def entropy_clustering(probs, cluster_num=4):
    """entropy_clustering of dataset_splitter.py:191-214 (its histogram branch) on device probabilities [m, C]:
    -> (labels int64 [m], entropies [m]).  As there: every label starts at 1, a row in bin i of np.histogram(entropies,
    cluster_num)'s edges takes label i, and since every bin is treated as half-open the largest entropy (== the last edge)
    stays at 1.  The edges depend on the smallest and largest entropy only; those two values are read back and numpy forms
    the edges from them, in the entropies' dtype, exactly as for the whole array."""
    ops._need_gpu(probs)
    u = cal_probs2entropy(probs)
    ends = torch.stack((u.min(), u.max())).cpu().numpy()
    edges = torch.as_tensor(np.histogram(ends, bins=cluster_num)[1]).to(device=u.device, dtype=u.dtype)
    labels = torch.ones(u.shape[0], dtype=torch.int64, device=u.device)
    for i in range(cluster_num):
        labels = torch.where((u >= edges[i]) & (u < edges[i + 1]), torch.full_like(labels, i), labels)
    return labels, u


def _subset_indices(indices, cluster_labels, swap=None, subset_fullsize=False):
    """Which clouds go to subset_1 / subset_2 (utils/train_files_spliter.py:212-226 with load_splitter_npy_list's 'random'
    choice): per class one cluster to each subset, cluster 0 to subset_1 unless swap[cls] is true (the reference shuffles
    the two file names); subset_fullsize (SUBSET_FULLSIZE): subset_2 is the whole class, subset_1's cluster first, as the
    shuffled file list concatenates.  indices / cluster_labels: per class index tensors (any device) -> two index tensors,
    classes in ascending order, clouds in the sorted order the splitter saved them in."""
    first, second = [], []
    for cls, (idx, cl) in enumerate(zip(indices, cluster_labels)):
        k = 1 if (swap is not None and swap[cls]) else 0
        a, b = idx[cl == k], idx[cl != k]
        first.append(a)
        second.append(torch.cat((a, b)) if subset_fullsize else b)
    return torch.cat(first), torch.cat(second)


def as_dataset_spliter(pts, labels, split, swap=None, subset_fullsize=False):
    """The dictionary split_dataset() returns for METHOD 'Geometric' / 'Geo_hist' (utils/train_files_spliter.py:242-253),
    from a GeometricSplit and _subset_indices(): {"subset_1": {"pts", "label"}, "subset_2": {...}} as device tensors, what
    create_splitted_dataset hands to UnifiedPointDG subset by subset."""
    ops._need_gpu(pts, *split.indices)
    lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).astype(np.int64)).to(pts.device)
    one, two = _subset_indices(split.indices, split.cluster_labels, swap, subset_fullsize)
    return {name: {'pts': pts.index_select(0, idx), 'label': lab.index_select(0, idx)}
            for name, idx in (('subset_1', one), ('subset_2', two))}
