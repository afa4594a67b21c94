"""Source-only Point Transformer classifier (mirror of the reference's model/Ptran_model.py; train_source.py:6, :78-79
imports PointTransformerCls from there).

`Backbone` is PTran_g's encoder without the conv1d node branch (the same fc1 lift, transformer blocks, FPS / kNN
transition-downs and HIP kernels); `PointTransformerCls` puts `fc2(points.mean(1))` on it, through the fused head
(ops.ptcls_head) where the shapes allow and the composed library ops otherwise.  Module and parameter names follow the
reference, so its state_dict loads with strict=True.  `TransitionUp` is the decoder's up-sampling step (two per-point
Linear + BatchNorm + ReLU branches and the 3-NN interpolation of feature propagation).
"""
import torch.nn as nn

from .. import ops
from .Model import PTran_g, TransitionDown, _check_input
from .PTran_utils import PointNetFeaturePropagation
from .Ptran_transformer import TransformerBlock

# the reference's defaults (Ptran_model.py:98-104)
_DEFAULTS = {'num_point': 1024, 'num_class': 10, 'input_dim': 3,
             'model': {'nneighbor': 16, 'nblocks': 4, 'transformer_dim': 512}}
# what the Point Transformer kernels run: xyz input only, k = 16 neighbours, four transition-downs, d_model = 512
_SUPPORTED = (('input_dim', 3), ('model.nneighbor', 16), ('model.nblocks', 4), ('model.transformer_dim', 512))


def _get(cfg, path):
    """cfg field `a.b`: attribute access (EasyDict, any namespace object) or keys of a plain nested dict."""
    for name in path.split('.'):
        cfg = cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)
    return cfg


def _settings(cfg):
    """(num_point, nblocks, nneighbor, num_class, input_dim, transformer_dim) of a cfg, checked against what runs here."""
    cfg = _DEFAULTS if cfg is None else cfg
    for path, want in _SUPPORTED:
        got = _get(cfg, path)
        if got != want:
            raise NotImplementedError('PointTransformerCls: cfg.%s = %r is not supported by the Point Transformer kernels '
                                      '(supported: %s = %d)' % (path, got, path, want))
    npoints, n_c = int(_get(cfg, 'num_point')), int(_get(cfg, 'num_class'))
    if npoints // 4 ** 4 < 1:
        raise NotImplementedError('PointTransformerCls: cfg.num_point = %d leaves no point after four transition-downs '
                                  '(supported: num_point >= 256)' % npoints)
    if n_c < 1:
        raise ValueError('PointTransformerCls: cfg.num_class = %d' % n_c)
    return npoints, 4, 16, n_c, 3, 512


class _SwapAxes(nn.Module):
    """Holds nothing: keeps the reference's Sequential positions (Ptran_model.py:20-25), so the keys are fc?.0.* / fc?.2.*."""

    def forward(self, x):
        return x.transpose(1, 2)


class TransitionUp(nn.Module):
    """Ptran_model.py:18-48: feats1 = relu(bn(fc1(points1))) on the coarse level, interpolated onto the dense level's
    points (direct-form 3-NN, ops.fp_interp), plus feats2 = relu(bn(fc2(points2))).  Rows in and out."""

    def __init__(self, dim1, dim2, dim_out):
        super().__init__()
        self.fc1 = nn.Sequential(nn.Linear(dim1, dim_out), _SwapAxes(), nn.BatchNorm1d(dim_out), _SwapAxes(), nn.ReLU())
        self.fc2 = nn.Sequential(nn.Linear(dim2, dim_out), _SwapAxes(), nn.BatchNorm1d(dim_out), _SwapAxes(), nn.ReLU())
        self.fp = PointNetFeaturePropagation(-1, [])

    @staticmethod
    def _branch(fc, x):
        return ops.bn_act_rows(ops.linear_rows(x, fc[0].weight, fc[0].bias), fc[2], 0.0)

    def forward(self, xyz1, points1, xyz2, points2):
        """xyz1 [B,n1,3], points1 [B,n1,dim1] (coarse), xyz2 [B,n2,3], points2 [B,n2,dim2] (dense) -> [B,n2,dim_out]."""
        feats1 = self._branch(self.fc1, points1)
        feats2 = self._branch(self.fc2, points2)
        return self.fp.rows(xyz2, xyz1, None, feats1) + feats2


class Backbone(nn.Module):
    """Ptran_model.py:51-91: fc1 (3 -> 32 -> 32), transformer1, then four (TransitionDown, TransformerBlock) stages with the
    FPS schedule num_point // 4, // 16, // 64, // 256 (256/64/16/4 at num_point 1024, whatever the cloud size)."""

    def __init__(self, cfg=None):
        super().__init__()
        npoints, nblocks, nneighbor, n_c, d_points, d_model = _settings(cfg)
        self.fc1 = nn.Sequential(nn.Linear(d_points, 32), nn.ReLU(), nn.Linear(32, 32))
        self.transformer1 = TransformerBlock(32, d_model, nneighbor)
        self.transition_downs = nn.ModuleList()
        self.transformers = nn.ModuleList()
        for i in range(nblocks):
            channel = 32 * 2 ** (i + 1)
            self.transition_downs.append(TransitionDown(npoints // 4 ** (i + 1), nneighbor, [channel // 2 + 3, channel, channel]))
            self.transformers.append(TransformerBlock(channel, d_model, nneighbor))
        self.nblocks = nblocks

    def forward(self, x):
        """x [B,3,N,1] -> (points [B,4,512], [(xyz, features)] of the five levels, rows [B,n,3] / [B,n,C])."""
        _check_input(x)
        x_ = ops.cloud_rows(x)                                        # [B,N,3]
        xyz = x_[..., :3]
        points = self.transformer1(xyz, PTran_g._lift(self, x_))[0]
        xyz_and_feats = [(xyz, points)]
        for i in range(self.nblocks):
            xyz, points = self.transition_downs[i](xyz, points)
            points = self.transformers[i](xyz, points)[0]
            xyz_and_feats.append((xyz, points))
        return points, xyz_and_feats


class PointTransformerCls(nn.Module):
    """Ptran_model.py:94-117: Backbone, then fc2 = Linear(512, 256), ReLU, Linear(256, 64), ReLU, Linear(64, num_class) on
    the mean of the last level's points.  cfg: None (the reference's defaults), an attribute object (EasyDict) or a
    nested dict with num_point, num_class, input_dim and model.{nneighbor, nblocks, transformer_dim}."""

    def __init__(self, cfg=None):
        super().__init__()
        _, nblocks, _, n_c, _, _ = _settings(cfg)
        self.backbone = Backbone(cfg)
        self.fc2 = nn.Sequential(nn.Linear(32 * 2 ** nblocks, 256), nn.ReLU(), nn.Linear(256, 64), nn.ReLU(), nn.Linear(64, n_c))
        self.nblocks = nblocks

    def forward(self, x):
        """x [B,3,N,1] -> logits [B,num_class]."""
        points, _ = self.backbone(x)
        return classify(self.fc2, points)


def classify(fc2, points):
    """fc2(points.mean(1)): the fused head (ops.ptcls_head) where ops.ptcls_head_supported allows it (B <= 128,
    2 <= num_class <= 64, SUG_PTCLS_HEAD_FUSED not 0), the composed library ops otherwise."""
    if ops.ptcls_head_supported(points, fc2):
        l1, l2, l3 = fc2[0], fc2[2], fc2[4]
        return ops.ptcls_head(points, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    return fc2(points.mean(1))


__all__ = ['TransitionDown', 'TransitionUp', 'Backbone', 'PointTransformerCls']
