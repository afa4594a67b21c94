"""data/dataloader.py on the device: UnifiedPointDG keeps its clouds in HBM and produces a batch with one launch of
sug_prepare_batch; DeviceLoader stands where the trainer builds torch.utils.data.DataLoader(dataset, ...).

What the trainer holds after `data.to(device)` / `label.to(device).long()` is what batch() returns: data
[B, 3, N, 1] fp32 and label [B] int64 on the device.  Reading files and DistributedSampler stay with the caller
(create_single_dataset / create_splitted_dataset are not mirrored): hand the arrays they load to UnifiedPointDG, or
split one resident array into two sub-domains with sug_amd.dataset_splitter first.
"""
import numpy as np
import torch

from .. import ops


def _kl_div(x, y):
    """scipy.special.kl_div, elementwise: x log(x / y) - x + y (y for x == 0)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(x > 0, x * np.log(x / y) - x + y, y)


def kl_divergence_distance_(x, y):
    return _kl_div(x, y) * 0.5 + _kl_div(y, x) * 0.5


def class_indices(labels, class_num=10):
    """Per class the list of its sample indices (UnifiedPointDG.classes())."""
    indices = [[] for _ in range(class_num)]
    for i, label in enumerate(labels):
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


class UnifiedPointDG:
    """The reference's constructor plus `device` (default: the current HIP device, or that of `pts`) and `seed` (the key
    of the in-kernel generator; give the source and the target set different seeds).  `pts` [M, P, C>=3], a numpy
    array or a tensor: xyz is uploaded once as fp32.  Every batch advances the device-resident batch counter by one, so
    a run is reproducible from `seed` and no two batches share a draw."""

    def __init__(self, dataset_type, pts, labels, status='train', pc_input_num=1024, aug=True, model="DGCNN", device=None,
                 seed=0):
        if device is None:
            device = pts.device if torch.is_tensor(pts) and pts.is_cuda else torch.device('cuda')
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('UnifiedPointDG keeps its clouds on a HIP device only (got %s); there is no CPU fallback' % device)
        self.num_points = pc_input_num
        self.status = status
        self.aug = aug
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

        self.class_num = 10
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
        data = ops.prepare_batch(self.pts, idx.contiguous(), self.num_points, self.pre_rotate, self.aug, seed=self.seed,
                                 counter=self.counter, out=out)
        self.counter.add_(1)
        return data.unsqueeze(-1), self.labels_dev.index_select(0, idx)

    def __getitem__(self, index):
        data, _ = self.batch([int(index)])
        return data[0], self.labels[index]

    def __len__(self):
        return self.pts.shape[0]


class DeviceLoader:
    """Stands in for DataLoader(dataset, batch_size=.., shuffle=.., drop_last=..) and DataLoader(dataset,
    batch_sampler=..) over a UnifiedPointDG: same number and composition of batches.  The shuffle order comes from a
    host torch.Generator seeded with the dataset's seed (one randperm per epoch).  An epoch's index order goes to the
    device in one copy; a batch is a slice of it, one kernel launch and a label gather -- no host wait."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, batch_sampler=None):
        if batch_sampler is not None and (batch_size != 1 or shuffle or drop_last):
            raise ValueError('batch_sampler option is mutually exclusive with batch_size, shuffle, and drop_last')
        self.dataset = dataset
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.drop_last = drop_last
        self.batch_sampler = batch_sampler
        self.generator = torch.Generator().manual_seed(dataset.seed)

    def __len__(self):
        if self.batch_sampler is not None:
            return len(self.batch_sampler)
        n = len(self.dataset)
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
