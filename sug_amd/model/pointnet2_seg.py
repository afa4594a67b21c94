"""PointNet++ part segmentation (multi-scale grouping encoder, three feature propagations, a per-point head) over the HIP
kernels: the network the PointNet++ authors train on ShapeNet-Part, composed from pointnet2_utils' classes.

  sa1, sa2 (multi-scale grouping) -> sa3 (one group of all points) -> fp3, fp2 -> fp1 with points1 = [one-hot category, xyz,
  extra channels] -> conv1 / bn1 / ReLU / drop1 / conv2 on rows -> raw logits [B, N, num_part].

Eager only: the model is not captured into a hipGraph.  The farthest-point starts come from ops.draw_start -- the
CPU generator, one draw per multi-scale level -- as PointNetSetAbstractionMsg already takes them.
"""
import torch
import torch.nn as nn

from .. import ops
from .pointnet2_utils import PointNetFeaturePropagation, PointNetSetAbstraction, PointNetSetAbstractionMsg


class Pointnet2PartSeg(nn.Module):
    graph_capturable = False          # eager path only

    def __init__(self, num_part=50, num_category=16, extra_channels=0, npoint1=512, npoint2=128, dropout=0.5):
        super(Pointnet2PartSeg, self).__init__()
        self.num_part, self.num_category, self.extra_channels = int(num_part), int(num_category), int(extra_channels)
        self.npoint1 = int(npoint1)
        e = self.extra_channels
        self.sa1 = PointNetSetAbstractionMsg(npoint1, [0.1, 0.2, 0.4], [32, 64, 128], e, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = PointNetSetAbstractionMsg(npoint2, [0.4, 0.8], [64, 128], 320, [[128, 128, 256], [128, 196, 256]])
        self.sa3 = PointNetSetAbstraction(None, None, None, 515, [256, 512, 1024], group_all=True)
        self.fp3 = PointNetFeaturePropagation(1536, [256, 256])
        self.fp2 = PointNetFeaturePropagation(576, [256, 128])
        self.fp1 = PointNetFeaturePropagation(128 + self.num_category + 3 + e, [128, 128])
        self.conv1 = nn.Conv1d(128, 128, 1)
        self.bn1 = nn.BatchNorm1d(128)
        self.drop1 = nn.Dropout(dropout)
        self.conv2 = nn.Conv1d(128, self.num_part, 1)

    def _check_input(self, points, category):
        """The GPU-only contract at the model boundary, as Model._check_input states it for Net_MDA."""
        if not points.is_cuda or points.dtype != torch.float32:
            raise RuntimeError('sug_amd Pointnet2PartSeg runs on a HIP device with fp32 clouds [B,%d,N] only (got %s on %s): '
                               'there is no CPU / eager fallback; move the model and the batch to the GPU (.cuda())'
                               % (3 + self.extra_channels, points.dtype, points.device))
        ops._need_gpu(category)
        if points.dim() != 3 or points.shape[1] != 3 + self.extra_channels:
            raise RuntimeError('Pointnet2PartSeg expects clouds as [B,%d,N], got %s' % (3 + self.extra_channels, tuple(points.shape)))
        if points.shape[2] < self.npoint1:
            raise RuntimeError('Pointnet2PartSeg: N = %d points, fewer than npoint1 = %d' % (points.shape[2], self.npoint1))
        if category.dtype != torch.int64 or category.shape != (points.shape[0],):
            raise RuntimeError('Pointnet2PartSeg: category int64 [B] (got %s %s)' % (tuple(category.shape), category.dtype))

    def forward(self, points, category):
        """points [B, 3 + extra_channels, N] fp32, category [B] int64 -> (logits [B, N, num_part], global_feature [B, 1024])."""
        self._check_input(points, category)
        B, _, N = points.shape
        rows = points.permute(0, 2, 1)
        xyz = rows[:, :, :3].contiguous()
        extra = rows[:, :, 3:].contiguous() if self.extra_channels else None
        x1, f1 = self.sa1.rows(xyz, extra)
        x2, f2 = self.sa2.rows(x1, f1)
        x3, f3 = self.sa3.rows(x2, f2)
        f2 = self.fp3.rows(x2, x3, f2, f3)
        f1 = self.fp2.rows(x1, x2, f1, f2)
        # one-hot of the category by comparison (a category outside [0, num_category) gives a zero row, never an
        # out-of-bounds write), broadcast over the points: no host wait
        onehot = (category.view(B, 1) == torch.arange(self.num_category, device=points.device).view(1, -1)).to(torch.float32)
        parts = [onehot.view(B, 1, -1).expand(B, N, -1), xyz] + ([extra] if extra is not None else [])
        f0 = self.fp1.rows(xyz, x1, torch.cat(parts, dim=-1), f1)
        h = ops.bn_act_rows(ops.linear_rows(f0, self.conv1.weight.view(128, 128), self.conv1.bias), self.bn1, 0.0)
        h = self.drop1(h)
        logits = ops.linear_rows(h, self.conv2.weight.view(self.num_part, 128), self.conv2.bias)
        return logits, f3.reshape(B, -1)
