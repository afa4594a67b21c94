"""KPConv blocks (mirror of the reference's model/KPConv_blocks.py): the rigid / linear-influence / sum-aggregation
kernel point convolution, the per-cloud instance norm the reference calls BatchNormBlock, the unary, simple and
bottleneck blocks, max pooling and the global average.  Module, parameter and state_dict names match the reference; the
arithmetic runs in the HIP kernels of sug_amd/csrc/kpconv.hip (sug_amd.ops.kpconv, seg_instnorm, seg_max_pool,
seg_mean).

Where the reference passes `stack_lengths` (per-cloud row counts) this build passes the level's int32 device offsets
[B+1] (the `offsets` entry of the preprocessing dict): the kernels take the segments from device memory, without a host
synchronisation.  Only the rigid / linear / sum path is built; the other options raise NotImplementedError.

A level tensor may have more rows than its offsets name (PreprocessorGPU with level caps holds every level at a static
number of rows): the ops read the valid row counts from the offsets on the device and keep the dead rows exactly zero.
"""
import functools
import math

import numpy as np
import torch
import torch.nn as nn
from torch.nn.parameter import Parameter
from torch.nn.init import kaiming_uniform_

from .. import ops


# ----------------------------------------------------------------------------------------------- kernel dispositions
@functools.lru_cache(maxsize=None)
def _repulsion_disposition(K, dimension=3, fixed='center', steps=400, seed=42):
    """K points in the unit ball, point 0 at the centre when fixed == 'center': gradient descent on the energy
    sum_{i<j} 1/|x_i - x_j| + sum_i |x_i|^2 (repulsion between points, attraction to the centre), the moving points
    projected back into the ball after every step.  Deterministic (its own generator, fp64)."""
    if fixed not in ('center', 'none'):
        raise NotImplementedError("kernel dispositions: fixed='%s' is not built (only 'center' and 'none')" % fixed)
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(K, dimension, generator=g, dtype=torch.float64) * 2 - 1
    x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-9) * torch.rand(K, 1, generator=g, dtype=torch.float64) ** (1 / 3)
    if fixed == 'center':
        x[0] = 0
    lr = 0.05
    for it in range(steps):
        x.requires_grad_(True)
        d = (x.unsqueeze(0) - x.unsqueeze(1)).norm(dim=2) + torch.eye(K, dtype=torch.float64)
        e = (1.0 / d).triu(1).sum() + (x * x).sum()
        (gr,) = torch.autograd.grad(e, x)
        with torch.no_grad():
            step = gr / gr.norm(dim=1, keepdim=True).clamp_min(1e-12)
            x = x - lr * (1 - it / steps) * step
            if fixed == 'center':
                x[0] = 0
            n = x.norm(dim=1, keepdim=True)
            x = torch.where(n > 1, x / n, x)
    return x.detach()


def load_kernels(radius, num_kpoints, dimension, fixed, lloyd=False):
    """model/KPConv_kernels.py load_kernels: a kernel disposition of `num_kpoints` points in the ball of `radius`, at a
    random rotation.  The reference reads an optimised disposition from a .ply file of its own tree; this build optimises
    its own (_repulsion_disposition, a fixed seed) and draws the rotation from torch's CPU generator.  Checkpoints carry
    the kernel points (a non-trainable parameter), so parity never depends on this choice."""
    if dimension != 3:
        raise NotImplementedError('kernel dispositions: only 3-D kernels are built')
    kp = _repulsion_disposition(num_kpoints, dimension, fixed).clone()
    theta = torch.rand(1).item() * 2 * math.pi
    phi = (torch.rand(1).item() - 0.5) * math.pi
    u = np.array([math.cos(theta) * math.cos(phi), math.sin(theta) * math.cos(phi), math.sin(phi)])
    alpha = torch.rand(1).item() * 2 * math.pi
    ux = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    R = math.cos(alpha) * np.eye(3) + math.sin(alpha) * ux + (1 - math.cos(alpha)) * np.outer(u, u)    # Rodrigues
    return (kp.numpy() @ R.T * radius).astype(np.float32)


# ----------------------------------------------------------------------------------------------- helpers
def _rev_single(neighb_inds, Nq, Ns):
    """(reverse lists, query offsets) of a neighbour table treated as one cloud (a KPConv called outside the preprocessed
    batch)."""
    if Ns > ops.KPCONV_MAX_CLOUD:
        raise NotImplementedError('KPConv outside a preprocessed batch: at most %d supports (got %d)' % (ops.KPCONV_MAX_CLOUD, Ns))
    dev = neighb_inds.device
    qoff = torch.tensor([0, Nq], dtype=torch.int32, device=dev)
    soff = torch.tensor([0, Ns], dtype=torch.int32, device=dev)
    return ops.radius_reverse(neighb_inds, qoff, soff, Ns, max(Ns, 1)), qoff


def _i32(t):
    return (t if t.dtype == torch.int32 else t.to(torch.int32)).contiguous()


def max_pool(x, inds, rev=None):
    """[n2, d]: max over each row's pooling slots of x (shadow slot = 0 row), model/KPConv_blocks.py:127-142."""
    inds = _i32(inds)
    if rev is None:
        rev, _ = _rev_single(inds, inds.shape[0], x.shape[0])
    return ops.seg_max_pool(x, inds, rev)


def global_average(x, batch_offsets):
    """[B, d]: per-cloud mean of the rows of x (model/KPConv_blocks.py:179-197); batch_offsets [B+1] int32 (device)."""
    return ops.seg_mean(x, batch_offsets)


def sample_index(lengths, sampled_len=64):
    """Row indices (into the packed level) of sample_tensor_slices (model/KPConv_blocks.py:159-176) for host lengths."""
    idx, i0 = [], 0
    for n in lengths:
        n = int(n)
        if n < sampled_len:
            local = list(range(n)) * (sampled_len // n) + list(range(sampled_len % n))
        else:
            local = list(range(0, n, n // sampled_len))[:sampled_len]
        idx.extend(i0 + j for j in local)
        i0 += n
    return idx


def sample_tensor_slices(x, batch_lengths, sampled_len=64):
    """[B, sampled_len, d]: the rows sample_tensor_slices of the reference picks per cloud (an even stride, or the cloud
    repeated when it is shorter), gathered on the device by sug_gather_rows.  batch_lengths: host ints."""
    idx = sample_index(batch_lengths, sampled_len)
    it = torch.tensor(idx, dtype=torch.int32).to(x.device, non_blocking=True)
    out = ops.gather_rows(x.unsqueeze(0), it.view(1, -1))
    return out.view(len(batch_lengths), sampled_len, x.shape[1])


# ----------------------------------------------------------------------------------------------- KPConv
class KPConv(nn.Module):

    def __init__(self, kernel_size, p_dim, in_channels, out_channels, KP_extent, radius,
                 fixed_kernel_points='center', KP_influence='linear', aggregation_mode='sum',
                 deformable=False, modulated=False):
        super(KPConv, self).__init__()
        if deformable or modulated:
            raise NotImplementedError('KPConv: deformable / modulated kernel points are not built (rigid kernels only)')
        if aggregation_mode != 'sum':
            raise NotImplementedError("KPConv: aggregation_mode '%s' is not built (only 'sum')" % aggregation_mode)
        if KP_influence != 'linear':
            raise NotImplementedError("KPConv: KP_influence '%s' is not built (only 'linear')" % KP_influence)
        if p_dim != 3:
            raise NotImplementedError('KPConv: only 3-D points are built')
        self.K = kernel_size
        self.p_dim = p_dim
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.radius = radius
        self.KP_extent = KP_extent
        self.fixed_kernel_points = fixed_kernel_points
        self.KP_influence = KP_influence
        self.aggregation_mode = aggregation_mode
        self.deformable = deformable
        self.modulated = modulated
        self.min_d2 = None
        self.deformed_KP = None
        self.offset_features = None
        self.weights = Parameter(torch.zeros((self.K, in_channels, out_channels), dtype=torch.float32), requires_grad=True)
        self.offset_dim = None
        self.offset_conv = None
        self.offset_bias = None
        self.reset_parameters()
        self.kernel_points = self.init_KP()

    def reset_parameters(self):
        kaiming_uniform_(self.weights, a=math.sqrt(5))

    def init_KP(self):
        K_points_numpy = load_kernels(self.radius, self.K, dimension=self.p_dim, fixed=self.fixed_kernel_points)
        return Parameter(torch.tensor(K_points_numpy, dtype=torch.float32), requires_grad=False)

    def forward(self, q_pts, s_pts, neighb_inds, x, rev=None, qoff=None):
        """[Nq, out_channels]; rev: the sorted reverse lists of neighb_inds (ops.radius_reverse), qoff: the query level's
        device offsets.  Without the two (the reference's call) the tables are one cloud's and both are built here."""
        neighb_inds = _i32(neighb_inds)
        if rev is None:
            rev, qoff = _rev_single(neighb_inds, q_pts.shape[0], s_pts.shape[0])
        return ops.kpconv(x, q_pts.contiguous(), s_pts.contiguous(), neighb_inds, rev, self.kernel_points, self.weights,
                          self.KP_extent, qoff)

    def __repr__(self):
        return 'KPConv(radius: {:.2f}, extent: {:.2f}, in_feat: {:d}, out_feat: {:d})'.format(
            self.radius, self.KP_extent, self.in_channels, self.out_channels)


# ----------------------------------------------------------------------------------------------- blocks
def block_decider(block_name, radius, in_dim, out_dim, layer_ind, config):
    if block_name == 'unary':
        return UnaryBlock(in_dim, out_dim, config.use_batch_norm, config.batch_norm_momentum)
    if block_name in ('simple', 'simple_strided'):
        return SimpleBlock(block_name, in_dim, out_dim, radius, layer_ind, config)
    if block_name in ('resnetb', 'resnetb_strided'):
        return ResnetBottleneckBlock(block_name, in_dim, out_dim, radius, layer_ind, config)
    if block_name == 'global_average':
        from .KPConv_model import GlobalAverageBlock
        return GlobalAverageBlock()
    raise NotImplementedError('KPConv block %r is not built (deformable, invariant / equivariant, pooling-only and '
                              'decoder blocks are out of scope)' % block_name)


class BatchNormBlock(nn.Module):
    """The reference's BatchNormBlock with use_bn: an InstanceNorm1d per cloud (biased variance, eps 1e-5, no affine
    parameters, no running buffers -- train and eval mode compute the same)."""

    def __init__(self, in_dim, use_bn, bn_momentum):
        super(BatchNormBlock, self).__init__()
        if not use_bn:
            raise NotImplementedError('BatchNormBlock(use_bn=False) (a bias instead of the instance norm) is not built')
        self.bn_momentum = bn_momentum
        self.use_bn = use_bn
        self.in_dim = in_dim
        self.norm = nn.InstanceNorm1d(in_dim, momentum=bn_momentum)

    def forward(self, x, stack_lengths, act=False, shortcut=None):
        """stack_lengths: the level's device offsets [B+1] (int32).  act: LeakyReLU(0.1) after the norm;
        shortcut: LeakyReLU(0.1)(norm + shortcut) (the end of the bottleneck block)."""
        return ops.seg_instnorm(x, stack_lengths, act=act, shortcut=shortcut)

    def __repr__(self):
        return 'BatchNormBlock(in_feat: {:d}, momentum: {:.3f}, only_bias: {:s})'.format(
            self.in_dim, self.bn_momentum, str(not self.use_bn))


class UnaryBlock(nn.Module):

    def __init__(self, in_dim, out_dim, use_bn, bn_momentum, no_relu=False):
        super(UnaryBlock, self).__init__()
        self.bn_momentum = bn_momentum
        self.use_bn = use_bn
        self.no_relu = no_relu
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.mlp = nn.Linear(in_dim, out_dim, bias=False)
        self.batch_norm = BatchNormBlock(out_dim, self.use_bn, self.bn_momentum)
        if not no_relu:
            self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, x, stack_lengths=None, shortcut=None):
        """shortcut (no_relu blocks only): LeakyReLU(0.1)(block(x) + shortcut) in the norm's epilogue."""
        y = ops.linear_rows(x, self.mlp.weight)
        return self.batch_norm(y, stack_lengths, act=not self.no_relu, shortcut=shortcut)

    def __repr__(self):
        return 'UnaryBlock(in_feat: {:d}, out_feat: {:d}, BN: {:s}, ReLU: {:s})'.format(
            self.in_dim, self.out_dim, str(self.use_bn), str(not self.no_relu))


def _level(batch, layer_ind, strided):
    """(q_pts, s_pts, neighbour table, its reverse lists, query offsets) of a block."""
    if strided:
        return (batch['points'][layer_ind + 1], batch['points'][layer_ind], batch['pools'][layer_ind],
                batch['rev_pools'][layer_ind], batch['offsets'][layer_ind + 1])
    return (batch['points'][layer_ind], batch['points'][layer_ind], batch['neighbors'][layer_ind],
            batch['rev_neighbors'][layer_ind], batch['offsets'][layer_ind])


class SimpleBlock(nn.Module):

    def __init__(self, block_name, in_dim, out_dim, radius, layer_ind, config):
        super(SimpleBlock, self).__init__()
        current_extent = radius * config.KP_extent / config.conv_radius
        self.bn_momentum = config.batch_norm_momentum
        self.use_bn = config.use_batch_norm
        self.layer_ind = layer_ind
        self.block_name = block_name
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.KPConv = KPConv(config.num_kernel_points, config.in_points_dim, in_dim, out_dim // 2, current_extent, radius,
                             fixed_kernel_points=config.fixed_kernel_points, KP_influence=config.KP_influence,
                             aggregation_mode=config.aggregation_mode, deformable='deform' in block_name,
                             modulated=config.modulated)
        self.batch_norm = BatchNormBlock(out_dim // 2, self.use_bn, self.bn_momentum)
        self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, x, batch):
        q_pts, s_pts, nbr, rev, off = _level(batch, self.layer_ind, 'strided' in self.block_name)
        x = self.KPConv(q_pts, s_pts, nbr, x, rev=rev, qoff=off)
        return self.batch_norm(x, off, act=True)


class ResnetBottleneckBlock(nn.Module):

    def __init__(self, block_name, in_dim, out_dim, radius, layer_ind, config):
        super(ResnetBottleneckBlock, self).__init__()
        current_extent = radius * config.KP_extent / config.conv_radius
        self.bn_momentum = config.batch_norm_momentum
        self.use_bn = config.use_batch_norm
        self.block_name = block_name
        self.layer_ind = layer_ind
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.last_block = config.num_layers == layer_ind + 1
        if in_dim != out_dim // 4:
            self.unary1 = UnaryBlock(in_dim, out_dim // 4, self.use_bn, self.bn_momentum)
        else:
            self.unary1 = nn.Identity()
        self.KPConv = KPConv(config.num_kernel_points, config.in_points_dim, out_dim // 4, out_dim // 4, current_extent,
                             radius, fixed_kernel_points=config.fixed_kernel_points, KP_influence=config.KP_influence,
                             aggregation_mode=config.aggregation_mode, deformable='deform' in block_name,
                             modulated=config.modulated)
        self.batch_norm_conv = BatchNormBlock(out_dim // 4, self.use_bn, self.bn_momentum)
        self.unary2 = UnaryBlock(out_dim // 4, out_dim, self.use_bn, self.bn_momentum, no_relu=True)
        if in_dim != out_dim:
            self.unary_shortcut = UnaryBlock(in_dim, out_dim, self.use_bn, self.bn_momentum, no_relu=True)
        else:
            self.unary_shortcut = nn.Identity()
        self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, features, batch):
        strided = 'strided' in self.block_name
        off_pre = batch['offsets'][self.layer_ind]
        q_pts, s_pts, nbr, rev, off_post = _level(batch, self.layer_ind, strided)
        x = self.unary1(features, off_pre) if isinstance(self.unary1, UnaryBlock) else features
        x = self.KPConv(q_pts, s_pts, nbr, x, rev=rev, qoff=off_post)
        x = self.batch_norm_conv(x, off_post, act=True)
        shortcut = max_pool(features, nbr, rev) if strided else features
        if isinstance(self.unary_shortcut, UnaryBlock):
            shortcut = self.unary_shortcut(shortcut, off_post)
        # unary2 (Linear + norm, no ReLU), the residual sum and the LeakyReLU in one epilogue
        return self.unary2(x, off_post, shortcut=shortcut)
