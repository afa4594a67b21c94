"""data/dataloader.py on the device: UnifiedPointDG keeps its clouds in HBM and produces a batch with one launch of
sug_prepare_batch; DeviceLoader stands where the trainer builds torch.utils.data.DataLoader(dataset, ...).

What the trainer holds after `data.to(device)` / `label.to(device).long()` is what batch() returns: data
[B, 3, N, 1] fp32 and label [B] int64 on the device.  Reading files stays with the caller (create_single_dataset /
create_splitted_dataset are not mirrored): hand the arrays they load to UnifiedPointDG, or split one resident array into
two sub-domains with sug_amd.dataset_splitter first.  DistributedSampler / build_dataloader shard a dataset over ranks as
the reference's do (data/dataloader.py:16-69), with DeviceLoader in DataLoader's place.
"""
from collections.abc import Mapping

import numpy as np
import torch
from torch.utils.data import DistributedSampler as _DistributedSampler

from .. import ops
from ..utils import common_utils


def _kl_div(x, y):
    """scipy.special.kl_div, elementwise: x log(x / y) - x + y (y for x == 0)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(x > 0, x * np.log(x / y) - x + y, y)


def kl_divergence_distance_(x, y):
    return _kl_div(x, y) * 0.5 + _kl_div(y, x) * 0.5


def class_indices(labels, class_num=10):
    """Per class the list of its sample indices (UnifiedPointDG.classes()).  A label outside [0, class_num) is a ValueError."""
    indices = [[] for _ in range(class_num)]
    for i, label in enumerate(labels):
        if not 0 <= int(label) < class_num:
            raise ValueError('class_indices: label %d of sample %d is outside [0, class_num = %d)' % (int(label), i, class_num))
        indices[int(label)].append(i)
    return indices


def class_weights(counts, dataset_size, weighting="number_inverse", q_=None):
    """UnifiedPointDG.cls_wights on the per-class sample counts (host arithmetic, the reference's values)."""
    class_num = len(counts)
    if weighting == "number_inverse":
        raw = [1 / n for n in counts]
    elif weighting == "exp_inverse":
        raw = [np.exp(-n / dataset_size) for n in counts]
    elif weighting == "DLSA":
        if q_ is not None and type(q_) is not str:
            q = q_
        elif q_ is not None:
            # the symmetric KL between the class distribution and the uniform one
            uniform = np.ones(class_num, dtype=np.float32) / class_num
            current = np.array([n / sum(counts) for n in counts])
            q = kl_divergence_distance_(current, uniform).sum(0)
        else:
            q = 0.4
        raw = [np.power(n, -q) for n in counts]
    else:
        return [1 / class_num] * class_num
    return [r / sum(raw) for r in raw]


_AUG_DEFAULTS = {'rotate_z': None, 'jitter': (0.01, 0.05), 'scale': (0.8, 1.25), 'perturb': (0.06, 0.18), 'shift': 0.1}


def parse_aug(aug):
    """An `aug` mapping -> (stage bits behind the normalisation, keyword parameters of ops.prepare_batch_aug).  Keys:
    'rotate_z' (bool), 'jitter' (sigma, clip), 'scale' (scale_low, scale_high), 'perturb' (angle_sigma, angle_clip), 'shift'
    shift_range; True stands for the reference function's defaults, a missing key or False / None for off."""
    unknown = sorted(set(aug) - set(_AUG_DEFAULTS))
    if unknown:
        raise ValueError('aug: unknown key(s) %s; the stages are %s' % (', '.join(map(repr, unknown)), ', '.join(_AUG_DEFAULTS)))
    on = {k: (_AUG_DEFAULTS[k] if v is True else v) for k, v in aug.items() if v is not None and v is not False}
    stages, kw = 0, {}
    if 'rotate_z' in on:
        stages |= ops.PREP_ROTATE_Z
    if 'jitter' in on:
        stages |= ops.PREP_JITTER
        kw['sigma'], kw['clip'] = (float(v) for v in on['jitter'])
    if 'scale' in on:
        stages |= ops.PREP_SCALE
        kw['scale_low'], kw['scale_high'] = (float(v) for v in on['scale'])
    if 'perturb' in on:
        stages |= ops.PREP_PERTURB
        kw['angle_sigma'], kw['angle_clip'] = (float(v) for v in on['perturb'])
    if 'shift' in on:
        stages |= ops.PREP_SHIFT
        kw['shift_range'] = float(on['shift'])
    return stages, kw


class UnifiedPointDG:
    """The reference's constructor plus `device` (default: the current HIP device, or that of `pts`) and `seed` (the key
    of the in-kernel generator; give the source and the target set different seeds).  `pts` [M, P, C>=3], a numpy
    array or a tensor: xyz is uploaded once as fp32.  Every batch advances the device-resident batch counter by one, so
    a run is reproducible from `seed` and no two batches share a draw.  `aug`: True / False as in the reference (z-rotation
    and jitter), or a mapping that selects the stages of pc_augment and their parameters (parse_aug), e.g.
    {'rotate_z': True, 'jitter': (0.01, 0.05), 'scale': (0.8, 1.25), 'perturb': (0.06, 0.18), 'shift': 0.1}.
    `class_num` (the reference fixes PointDA-10's ten): the number of classes; classes() and cls_wights() have that many
    entries, and a label outside [0, class_num) is a ValueError."""

    def __init__(self, dataset_type, pts, labels, status='train', pc_input_num=1024, aug=True, model="DGCNN", device=None,
                 seed=0, class_num=10):
        if device is None:
            device = pts.device if torch.is_tensor(pts) and pts.is_cuda else torch.device('cuda')
        device = torch.device(device)
        if int(class_num) != class_num or class_num < 1:
            raise ValueError('UnifiedPointDG: class_num must be a positive integer (got %r)' % (class_num,))
        if device.type != 'cuda':
            raise RuntimeError('UnifiedPointDG keeps its clouds on a HIP device only (got %s); there is no CPU fallback' % device)
        self.num_points = pc_input_num
        self.status = status
        self.aug = aug
        self.aug_stages = parse_aug(aug) if isinstance(aug, Mapping) else None
        self.dataset_type = dataset_type
        self.model = model
        self.seed = int(seed)
        if len(pts.shape) != 3 or pts.shape[2] < 3:
            raise ValueError('pts must be [M, P, C>=3], got %s' % (tuple(pts.shape),))
        if pts.shape[1] > ops.PREP_MAX_POINTS:
            raise ValueError('at most %d points per cloud, got %d' % (ops.PREP_MAX_POINTS, pts.shape[1]))
        if pts.shape[1] < pc_input_num / 1.5:
            raise RuntimeWarning(f"Too few points {pts.shape[1]} for pc_input_num {pc_input_num}")
        xyz = torch.as_tensor(pts)[:, :, :3]                      # for ScanNet, only x-y-z features are used
        self.pts = xyz.to(device=device, dtype=torch.float32).contiguous()
        self.labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
        self.labels_dev = torch.as_tensor(self.labels.astype(np.int64)).to(device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.device = device

        self.class_num = int(class_num)
        self.dataset_size = pts.shape[0]
        self.indices = class_indices(self.labels, self.class_num)
        self.cls_num_counter = [len(cls_index) for cls_index in self.indices]

    def classes(self):
        return self.indices

    def cls_wights(self, weighting="number_inverse", q_=None):
        return class_weights(self.cls_num_counter, self.dataset_size, weighting, q_)

    @property
    def pre_rotate(self):
        return self.dataset_type != "modelnet" and self.model == "DGCNN"

    def batch(self, indices, out=None):
        """indices: a device int32 tensor [B] (no copy) or any host sequence -> (data [B, 3, N, 1] fp32, label [B] int64)."""
        if torch.is_tensor(indices):
            ops._need_gpu(indices)
            idx = indices if indices.dtype == torch.int32 else indices.to(torch.int32)
        else:
            idx = torch.as_tensor(np.asarray(indices, dtype=np.int32)).to(self.device, non_blocking=True)
        if self.aug_stages is None:
            data = ops.prepare_batch(self.pts, idx.contiguous(), self.num_points, self.pre_rotate, self.aug, seed=self.seed,
                                     counter=self.counter, out=out)
        else:
            stages, kw = self.aug_stages
            data = ops.prepare_batch_aug(self.pts, idx.contiguous(), self.num_points, self.pre_rotate, True, seed=self.seed,
                                         counter=self.counter, out=out, stages=ops.PREP_NORMALIZE | stages, **kw)
        self.counter.add_(1)
        return data.unsqueeze(-1), self.labels_dev.index_select(0, idx)

    def __getitem__(self, index):
        data, _ = self.batch([int(index)])
        return data[0], self.labels[index]

    def __len__(self):
        return self.pts.shape[0]


class DeviceLoader:
    """Stands in for DataLoader(dataset, batch_size=.., shuffle=.., drop_last=..) and DataLoader(dataset,
    batch_sampler=..) over a UnifiedPointDG -- or any dataset with `batch(indices)`, `seed`, `device` and `__len__`, such as
    partseg.PartSegDataset, whose batches are (points, category, label): same number and composition of batches.  The shuffle order comes from a
    host torch.Generator seeded with the dataset's seed (one randperm per epoch).  An epoch's index order goes to the
    device in one copy; a batch is a slice of it, one kernel launch and a label gather -- no host wait.  `sampler`: any
    iterable of indices with a length (a DistributedSampler: this rank's share), read once per epoch."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, batch_sampler=None, sampler=None):
        if batch_sampler is not None and (batch_size != 1 or shuffle or drop_last or sampler is not None):
            raise ValueError('batch_sampler option is mutually exclusive with batch_size, shuffle, sampler, and drop_last')
        if sampler is not None and shuffle:
            raise ValueError('sampler option is mutually exclusive with shuffle')
        self.sampler = sampler
        self.dataset = dataset
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.drop_last = drop_last
        self.batch_sampler = batch_sampler
        self.generator = torch.Generator().manual_seed(dataset.seed)

    def __len__(self):
        if self.batch_sampler is not None:
            return len(self.batch_sampler)
        n = len(self.dataset) if self.sampler is None else len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        dev = self.dataset.device
        if self.batch_sampler is not None:
            sizes = []
            flat = []
            for b in self.batch_sampler:
                sizes.append(len(b))
                flat.extend(b)
            order = torch.tensor(flat, dtype=torch.int32)
        else:
            if self.sampler is not None:
                order = torch.tensor(list(self.sampler), dtype=torch.int32)
                n = order.numel()
            else:
                n = len(self.dataset)
                order = (torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)).to(torch.int32)
            sizes = [self.batch_size] * (n // self.batch_size)
            if n % self.batch_size and not self.drop_last:
                sizes.append(n % self.batch_size)
        order = order.to(dev, non_blocking=True)
        start = 0
        for size in sizes:
            yield self.dataset.batch(order[start:start + size])
            start += size


class DistributedSampler(_DistributedSampler):
    """The reference's sampler (data/dataloader.py:16-36) over torch's: per epoch a randperm seeded with the epoch number
    (or the identity with shuffle=False), padded by wrapping around to num_replicas * ceil(len / num_replicas) entries,
    of which rank r takes every num_replicas-th from r on.  set_epoch(e) selects the permutation."""

    def __init__(self, dataset, num_replicas=None, rank=None, shuffle=True):
        super().__init__(dataset, num_replicas=num_replicas, rank=rank)
        self.shuffle = shuffle

    def __iter__(self):
        n = len(self.dataset)
        if self.shuffle:
            order = torch.randperm(n, generator=torch.Generator().manual_seed(self.epoch)).tolist()
        else:
            order = list(range(n))
        order = order + order[:self.total_size - n]
        share = order[self.rank:self.total_size:self.num_replicas]
        if len(order) != self.total_size or len(share) != self.num_samples:
            raise RuntimeError('DistributedSampler: %d of %d indices for rank %d of %d' % (len(share), len(order), self.rank,
                                                                                          self.num_replicas))
        return iter(share)


def build_dataloader(dataset, batch_size, dist, workers=4, seed=None, training=True, merge_all_iters_to_one_epoch=False,
                     total_epochs=0):
    """The reference's build_dataloader (data/dataloader.py:39-69) -> (dataset, DeviceLoader, sampler): drop_last=True;
    torch's DistributedSampler when `dist and training`, the class above without shuffling when `dist and not training`,
    no sampler and a shuffled loader (when training) otherwise.  `workers` and `seed` are accepted and ignored: there are
    no worker processes to start or seed, a batch is one kernel launch on the resident clouds."""
    if merge_all_iters_to_one_epoch:
        if not hasattr(dataset, 'merge_all_iters_to_one_epoch'):
            raise ValueError('build_dataloader: the dataset has no merge_all_iters_to_one_epoch')
        dataset.merge_all_iters_to_one_epoch(merge=True, epochs=total_epochs)
    sampler = None
    if dist and training:
        sampler = _DistributedSampler(dataset)
    elif dist:
        rank, world_size = common_utils.get_dist_info()
        sampler = DistributedSampler(dataset, world_size, rank, shuffle=False)
    loader = DeviceLoader(dataset, batch_size=batch_size, shuffle=sampler is None and training, drop_last=True, sampler=sampler)
    return dataset, loader, sampler
