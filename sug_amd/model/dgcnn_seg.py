"""DGCNN part segmentation over the HIP kernels: the network the DGCNN authors train on ShapeNet-Part, on point-major rows.

  kNN(xyz) -> transform_net (6 -> 64 -> 128, max over k, tail) -> x . T
  kNN(x)   -> conv1, conv2 (6 -> 64 -> 64), max over k -> x1          two-layer EdgeConv block (ops.edgeconv2)
  kNN(x1)  -> conv3, conv4 (128 -> 64 -> 64), max over k -> x2        two-layer EdgeConv block
  kNN(x2)  -> conv5 (128 -> 64), max over k -> x3                     single-layer EdgeConv (as conv_2d.edge_rows)
  conv6 on cat(x1, x2, x3) -> max over N -> g;  conv7 on the one-hot category -> l
  conv8 on cat([g | l] per cloud, x1, x2, x3) -> dp1 -> conv9 -> dp2 -> conv10 -> conv11 -> raw logits [B, N, num_part]

The input transform is the T-Net this package ships (model_utils.transform_net, LayerNorm in its FC tail), not the authors'
BatchNorm1d variant.  Eager only: the model is not captured into a hipGraph.
"""
import torch
import torch.nn as nn

from .. import ops
from .model_utils import transform_net

SLOPE = 0.2


def _w2(conv):
    w = conv.weight
    return w.view(w.shape[0], w.shape[1])


class DGCNNPartSeg(nn.Module):
    graph_capturable = False          # eager path only

    def __init__(self, num_part=50, num_category=16, k=20, emb_dims=1024, dropout=0.5, input_transform=True):
        super(DGCNNPartSeg, self).__init__()
        self.num_part, self.num_category, self.k, self.emb_dims = int(num_part), int(num_category), int(k), int(emb_dims)
        self.input_transform = bool(input_transform)
        if self.input_transform:
            self.transform_net = transform_net(6, 3)
            nn.init.zeros_(self.transform_net.fc3.weight)      # the transform starts as the identity (the tail adds eye)
            nn.init.zeros_(self.transform_net.fc3.bias)
        act = lambda: nn.LeakyReLU(negative_slope=SLOPE)
        for i in range(1, 6):
            setattr(self, 'bn%d' % i, nn.BatchNorm2d(64))
        self.bn6 = nn.BatchNorm1d(self.emb_dims)
        self.bn7 = nn.BatchNorm1d(64)
        self.bn8 = nn.BatchNorm1d(256)
        self.bn9 = nn.BatchNorm1d(256)
        self.bn10 = nn.BatchNorm1d(128)
        self.conv1 = nn.Sequential(nn.Conv2d(6, 64, kernel_size=1, bias=False), self.bn1, act())
        self.conv2 = nn.Sequential(nn.Conv2d(64, 64, kernel_size=1, bias=False), self.bn2, act())
        self.conv3 = nn.Sequential(nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False), self.bn3, act())
        self.conv4 = nn.Sequential(nn.Conv2d(64, 64, kernel_size=1, bias=False), self.bn4, act())
        self.conv5 = nn.Sequential(nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False), self.bn5, act())
        self.conv6 = nn.Sequential(nn.Conv1d(192, self.emb_dims, kernel_size=1, bias=False), self.bn6, act())
        self.conv7 = nn.Sequential(nn.Conv1d(self.num_category, 64, kernel_size=1, bias=False), self.bn7, act())
        self.conv8 = nn.Sequential(nn.Conv1d(self.emb_dims + 64 + 192, 256, kernel_size=1, bias=False), self.bn8, act())
        self.dp1 = nn.Dropout(p=dropout)
        self.conv9 = nn.Sequential(nn.Conv1d(256, 256, kernel_size=1, bias=False), self.bn9, act())
        self.dp2 = nn.Dropout(p=dropout)
        self.conv10 = nn.Sequential(nn.Conv1d(256, 128, kernel_size=1, bias=False), self.bn10, act())
        self.conv11 = nn.Conv1d(128, self.num_part, kernel_size=1, bias=False)

    def _check_input(self, points, category):
        """The GPU-only contract at the model boundary, as Pointnet2PartSeg._check_input states it."""
        if not points.is_cuda or points.dtype != torch.float32:
            raise RuntimeError('sug_amd DGCNNPartSeg runs on a HIP device with fp32 clouds [B,3,N] only (got %s on %s): '
                               'there is no CPU / eager fallback; move the model and the batch to the GPU (.cuda())'
                               % (points.dtype, points.device))
        ops._need_gpu(category)
        if points.dim() != 3 or points.shape[1] != 3:
            raise RuntimeError('DGCNNPartSeg expects clouds as [B,3,N], got %s' % (tuple(points.shape),))
        if points.shape[2] < self.k:
            raise RuntimeError('DGCNNPartSeg: N = %d points, fewer than k = %d' % (points.shape[2], self.k))
        if category.dtype != torch.int64 or category.shape != (points.shape[0],):
            raise RuntimeError('DGCNNPartSeg: category int64 [B] (got %s %s)' % (tuple(category.shape), category.dtype))

    def _rows(self, seq, x):
        """Conv1d (no bias) -> BatchNorm1d -> LeakyReLU(0.2) of a Sequential on [..., Cin] rows."""
        return ops.bn_act_rows(ops.linear_rows(x, _w2(seq[0])), seq[1], SLOPE)

    def _edge1(self, seq, wcat, x, idx, out):
        """Single-layer EdgeConv with slope 0.2 (conv_2d.edge_rows' two paths; that class only names slope 0.01)."""
        B, N, C = x.shape
        bn = seq[1]
        Co = wcat.shape[0] // 2
        ops._count_bn_call(bn)
        if ops.edgeconv_fused_supported(N, idx.shape[2], C, Co):
            return ops.edgeconv_fused(x, wcat, None, idx, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training,
                                      SLOPE, bn.eps, bn.momentum, out=out)[0]
        pq = ops.linear_rows(x, wcat)
        return ops.edgeconv_bn_act_max(pq, idx, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, SLOPE,
                                       bn.eps, bn.momentum, out=out)[0]

    def forward(self, points, category, knn_idx=None, return_graphs=False):
        """points [B,3,N] fp32, category [B] int64 -> (logits [B,N,num_part], global feature [B,emb_dims]).
        knn_idx: four [B,N,k] int32 tensors that override the graphs of xyz, x . T, x1, x2 (tests: teacher forcing; the
        first is unused without the input transform).  return_graphs: also return the four lists the forward used."""
        self._check_input(points, category)
        B, _, N = points.shape
        k = self.k
        gi = list(knn_idx) if knn_idx is not None else [None] * 4
        if len(gi) != 4:
            raise RuntimeError('DGCNNPartSeg: knn_idx is four [B,N,k] int32 tensors')
        for t in gi:
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (B, N, k) or not t.is_cuda):
                raise RuntimeError('DGCNNPartSeg: knn_idx is four [B,N,k] int32 tensors on the device')
        used = [None] * 4

        def nb(f, i):
            used[i] = gi[i] if gi[i] is not None else ops.knn(f, k)
            return used[i]

        x = points.permute(0, 2, 1).contiguous()                               # [B,N,3] rows
        if self.input_transform:
            T = self.transform_net.edge_rows(x, nb(x, 0))                      # [B,3,3]
            x = torch.bmm(x, T)
        cat_in = torch.empty(B, N, 192, dtype=torch.float32, device=points.device)
        w1, w3, w5 = ops.edge_weight_split_multi([_w2(self.conv1[0]), _w2(self.conv3[0]), _w2(self.conv5[0])])
        # gradients reach T through linear_rows' backward of the first block's [P | Q]
        x1 = ops.edgeconv2(ops.linear_rows(x, w1), nb(x, 1), self.bn1, SLOPE, _w2(self.conv2[0]), None, self.bn2, SLOPE,
                           out=cat_in[:, :, 0:64])
        x2 = ops.edgeconv2(ops.linear_rows(x1, w3), nb(x1, 2), self.bn3, SLOPE, _w2(self.conv4[0]), None, self.bn4, SLOPE,
                           out=cat_in[:, :, 64:128])
        x3 = self._edge1(self.conv5, w5, x2, nb(x2, 3), cat_in[:, :, 128:192])
        feats = ops.assemble_rows(cat_in, (x1, x2, x3))                        # [B,N,192], no copy
        g = ops.bn_act_pool(ops.linear_rows(feats, _w2(self.conv6[0])), self.bn6, SLOPE)[0]      # [B,emb_dims]
        # one-hot of the category by comparison: no host wait, a category outside the range gives a zero row
        onehot = (category.view(B, 1) == torch.arange(self.num_category, device=points.device).view(1, -1)).to(torch.float32)
        l = self._rows(self.conv7, onehot)                                     # [B,64]
        # conv8 on cat([g | l] repeated over N, x1, x2, x3) without the [B,N,1280] tensor: the per-cloud columns once
        # per cloud, broadcast onto the per-point columns' product
        W8 = _w2(self.conv8[0])
        ng = self.emb_dims + 64
        cloud = ops.linear_rows(torch.cat((g, l), dim=1), W8[:, :ng].contiguous())                # [B,256]
        h = ops.linear_rows(feats, W8[:, ng:].contiguous()) + cloud.unsqueeze(1)
        h = self.dp1(ops.bn_act_rows(h, self.bn8, SLOPE))
        h = self.dp2(self._rows(self.conv9, h))
        h = self._rows(self.conv10, h)
        logits = ops.linear_rows(h, _w2(self.conv11))
        if return_graphs:
            return logits, g, used
        return logits, g
