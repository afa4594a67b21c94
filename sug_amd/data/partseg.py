"""The part-segmentation dataset on the device: PartSegDataset keeps its clouds (xyz, extra channels, per-point part labels,
lengths) in HBM and produces a batch -- (points [B, 3 + E, N], category [B], label [B, N]), what SegStep.step and
seg_eval_worker's tuples take -- with one launch of sug_prepare_seg_batch.  The usual host recipe
(np.random.choice(len, npoints, replace=True) per cloud, then normalise and augment) is replaced by: a random ordered subset
of a cloud longer than N, all the points of a shorter one followed by draws with replacement; every output row is a real
point with a real label, so PartIoUMeter scores every cloud.  Reading ShapeNet-Part files stays with the caller.
DeviceLoader / build_dataloader (dataloader.py) drive it unchanged.
"""
from collections.abc import Mapping

import numpy as np
import torch

from .. import ops
from ..utils.seg_utils import PartIoUMeter
from .dataloader import parse_aug

PARTSEG_AUG = {'scale': (0.8, 1.25), 'shift': 0.1}             # aug=True: the usual part-segmentation recipe


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def pack_clouds(clouds):
    """A list of M arrays [L_m, ...] (the same trailing shape and dtype family) -> (packed [M, max L_m, ...], zero rows behind
    each cloud's own; lengths [M] int32).  Pure host function."""
    clouds = [_host(c) for c in clouds]
    if not clouds:
        raise ValueError('pack_clouds: an empty list')
    tail = clouds[0].shape[1:]
    for m, c in enumerate(clouds):
        if c.ndim < 1 or c.shape[1:] != tail:
            raise ValueError('pack_clouds: cloud %d has shape %s, cloud 0 has [L, %s]' % (m, c.shape, ', '.join(map(str, tail))))
        if c.shape[0] < 1:
            raise ValueError('pack_clouds: cloud %d is empty' % m)
    lengths = np.array([c.shape[0] for c in clouds], dtype=np.int32)
    packed = np.zeros((len(clouds), int(lengths.max())) + tail, dtype=np.result_type(*[c.dtype for c in clouds]))
    for m, c in enumerate(clouds):
        packed[m, :c.shape[0]] = c
    return packed, lengths


class PartSegDataset:
    """pts [M, P, 3 + E] (or a list of M arrays [L_m, 3 + E], packed by pack_clouds), point_labels in the same outer layout,
    categories [M]; category k owns the parts [part_first[k], part_first[k] + part_count[k]).  lengths [M]: the valid points
    of each cloud (default: P, or the list's).  Everything is checked on the host once and uploaded once.
    aug: False -- normalise only; True -- PARTSEG_AUG; a mapping -- parse_aug's stages.  normals: channels 3..5 are a
    direction and turn with the cloud under every rotation stage (when E >= 3).  `seed` keys the in-kernel generator; every
    batch advances the device-resident counter by one."""

    def __init__(self, pts, point_labels, categories, part_first, part_count, lengths=None, num_points=2048, aug=False,
                 normals=True, seed=0, device=None):
        if device is None:
            device = pts.device if torch.is_tensor(pts) and pts.is_cuda else torch.device('cuda')
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('PartSegDataset keeps its clouds on a HIP device only (got %s); there is no CPU fallback' % device)
        if isinstance(pts, (list, tuple)):
            pts, own = pack_clouds(pts)
            point_labels, own_l = pack_clouds(point_labels) if isinstance(point_labels, (list, tuple)) else (point_labels, own)
            if not np.array_equal(own, own_l):
                m = int(np.flatnonzero(own != own_l)[0]) if len(own) == len(own_l) else min(len(own), len(own_l))
                raise ValueError('PartSegDataset: cloud %d: its points and its labels differ in length' % m)
            if lengths is None:
                lengths = own
        pts, lab, cat = _host(pts), _host(point_labels), _host(categories).reshape(-1)
        if pts.ndim != 3 or pts.shape[2] < 3:
            raise ValueError('PartSegDataset: pts must be [M, P, 3 + E], got %s' % (pts.shape,))
        M, P, C = pts.shape
        E = C - 3
        if E > ops.PREP_SEG_MAX_EXTRA:
            raise ValueError('PartSegDataset: at most %d extra channels, got %d' % (ops.PREP_SEG_MAX_EXTRA, E))
        if P > ops.PREP_MAX_POINTS:
            raise ValueError('PartSegDataset: at most %d points per cloud, got %d' % (ops.PREP_MAX_POINTS, P))
        if not 1 <= int(num_points) <= ops.PREP_MAX_POINTS:
            raise ValueError('PartSegDataset: num_points must be in [1, %d], got %r' % (ops.PREP_MAX_POINTS, num_points))
        if lab.shape != (M, P) or cat.shape != (M,):
            raise ValueError('PartSegDataset: point_labels must be [M, P] = [%d, %d] and categories [%d], got %s and %s'
                             % (M, P, M, lab.shape, cat.shape))
        lengths = np.full(M, P, dtype=np.int64) if lengths is None else _host(lengths).reshape(-1).astype(np.int64)
        if lengths.shape != (M,):
            raise ValueError('PartSegDataset: lengths must be [M] = [%d], got %s' % (M, lengths.shape))
        bad = np.flatnonzero((lengths < 1) | (lengths > P))
        if bad.size:
            raise ValueError('PartSegDataset: cloud %d has length %d, outside [1, P = %d]' % (bad[0], lengths[bad[0]], P))
        self.part_first, self.part_count = ops.part_table(part_first, part_count)
        K = int(self.part_first.shape[0])
        cat = cat.astype(np.int64)
        bad = np.flatnonzero((cat < 0) | (cat >= K))
        if bad.size:
            raise ValueError('PartSegDataset: cloud %d has category %d, outside [0, K = %d)' % (bad[0], cat[bad[0]], K))
        lab = lab.astype(np.int64)
        valid = np.arange(P)[None, :] < lengths[:, None]
        first, count = self.part_first.astype(np.int64)[cat][:, None], self.part_count.astype(np.int64)[cat][:, None]
        for what, wrong in (('is not below SUG_SEG_MAX_PARTS = %d' % ops.SEG_MAX_PARTS, (lab < 0) | (lab >= ops.SEG_MAX_PARTS)),
                            ('is outside the part range of its category', (lab < first) | (lab >= first + count))):
            wrong = wrong & valid
            if wrong.any():
                m, p = np.unravel_index(int(np.argmax(wrong)), wrong.shape)
                raise ValueError('PartSegDataset: label %d of point %d of cloud %d (category %d: parts [%d, %d)) %s'
                                 % (lab[m, p], p, m, cat[m], first[m, 0], first[m, 0] + count[m, 0], what))

        self.num_points = int(num_points)
        self.seed = int(seed)
        self.device = device
        self.aug = aug
        stages, self.aug_kw = parse_aug(aug if isinstance(aug, Mapping) else (PARTSEG_AUG if aug else {}))
        self.stages = ops.PREP_NORMALIZE | stages | (ops.PREP_NORMALS if normals and E >= 3 else 0)
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        self.pts = f32(pts[:, :, :3])
        self.extra = f32(pts[:, :, 3:]) if E else None
        self.point_labels = torch.as_tensor(np.where(valid, lab, 0).astype(np.uint8)).to(device)
        self.categories = torch.as_tensor(cat).to(device)
        self.lengths = torch.as_tensor(lengths.astype(np.int32)).to(device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.extra_channels = E

    def batch(self, indices, out=None):
        """indices: a device int32 tensor [B] (no copy) or any host sequence -> (points [B, 3 + E, N] fp32, category [B] int64,
        label [B, N] int64), SegStep.step's argument order.  out: three such tensors to write into (the batch is then one
        launch and nothing is allocated).  One counter increment; no host wait."""
        if torch.is_tensor(indices):
            ops._need_gpu(indices)
            idx = indices if indices.dtype == torch.int32 else indices.to(torch.int32)
        else:
            idx = torch.as_tensor(np.asarray(indices, dtype=np.int32)).to(self.device, non_blocking=True)
        points, category, label = (None, None, None) if out is None else out
        res = ops.prepare_seg_batch(self.pts, self.extra, self.point_labels, self.categories, self.lengths, idx.contiguous(),
                                    self.num_points, seed=self.seed, counter=self.counter, out=points, label_out=label,
                                    category_out=category, stages=self.stages, **self.aug_kw)
        self.counter.add_(1)
        return res

    def __getitem__(self, index):
        points, category, label = self.batch([int(index)])
        return points[0], category[0], label[0]

    def __len__(self):
        return self.pts.shape[0]

    def meter(self):
        """A PartIoUMeter on this dataset's part table and device."""
        return PartIoUMeter(self.part_first, self.part_count, self.device)
