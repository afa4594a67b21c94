"""KPConv encoder, preprocessing and classifier (mirror of the reference's model/KPConv_model.py).

PreprocessorGPU builds the whole pyramid on the device -- grid subsampling (sug_grid_subsample), radius neighbours,
pools and upsamples (sug_radius_neighbors) and the reverse lists the backward passes scatter through
(sug_radius_reverse) -- with ONE host synchronisation per forward: the copy of all level lengths, which the packed
sizes need.  The two third-party operations of the reference (MinkowskiEngine's quantisation, pytorch3d's ball_query)
are restated under documented assumptions:
  * radius query: per query, the first `limit` supports of its cloud in index order with d^2 < r^2, d^2 in fp32 as
    (s - q) per axis, summed x, y, z; r^2 = fp32(r) * fp32(r); missing slots hold the shadow index (total supports);
  * grid subsample: key = floor(fp32(p) / fp32(dl)) per axis (true division), voxels per cloud in order of their first
    point (MinkowskiEngine's own order is a hash order), the voxel point = fp32 sum in point order / count.

Every op takes level buffers of at least off[B] rows and reads the valid counts from the device offsets (kpconv.hip,
"ROW LAYOUT"); the exact-size pyramid slices its buffers to exactly off[B] rows.  With level caps (`set_level_caps` of
KPConv_g / KPFCls) level l instead keeps a buffer of a static number of rows (`level_capacity`), and nothing is
copied to the host -- a forward and its backward are one static launch sequence, which a hipGraph can replay.  A level
that needs more rows than its capacity is truncated (the tail of the last clouds) and noted in a small device record that
`capacity_report` reads; `calibrate_level_caps` measures caps on sample batches with the exact-size path.
"""
import math
from typing import List

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .KPConv_blocks import block_decider, global_average, UnaryBlock


class _Config(dict):
    """Attribute access over a dict (the reference's EasyDict)."""
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None       # (copy.deepcopy probes __deepcopy__: a KeyError would escape it)

    def __setattr__(self, k, v):
        self[k] = v


KPConvConfig = _Config()
KPConvConfig["num_class"] = 10
KPConvConfig["first_subsampling_dl"] = 0.02
KPConvConfig["conv_radius"] = 2.5
KPConvConfig["deform_radius"] = 6.0
KPConvConfig["d_bottle"] = 256
KPConvConfig["in_feats_dim"] = 1
KPConvConfig["KP_extent"] = 1.2
KPConvConfig["KP_influence"] = "linear"
KPConvConfig["overlap_radius"] = 0.04
KPConvConfig["use_batch_norm"] = True
KPConvConfig["batch_norm_momentum"] = 0.02
KPConvConfig["modulated"] = False
KPConvConfig["num_kernel_points"] = 15
KPConvConfig["first_feats_dim"] = 64
KPConvConfig["fixed_kernel_points"] = "center"
KPConvConfig["neighborhood_limits"] = [50, 50, 50, 50, 50]
KPConvConfig["aggregation_mode"] = "sum"
KPConvConfig["in_points_dim"] = 3
KPConvConfig["num_layers"] = 5
KPConvConfig["architecture"] = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb', 'resnetb_strided', 'resnetb',
                                'resnetb', 'resnetb_strided', 'resnetb', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb']
KPConvConfig["deform_fitting_power"] = 1.0


def _layer_plan(config):
    """[(radius, pooled at the end)] per level, as the reference's preprocessing loop walks the architecture."""
    for block in config.architecture:
        if 'upsample' in block or 'deform' in block:
            raise NotImplementedError('KPConv preprocessing: %r blocks are not built (no decoder, rigid kernels only)'
                                      % block)
    plan, r, blocks = [], config.first_subsampling_dl * config.conv_radius, []
    arch = config.architecture
    for i, block in enumerate(arch):
        if 'global' in block:
            break
        if not ('pool' in block or 'strided' in block):
            blocks.append(block)
            if i < len(arch) - 1:
                continue
        plan.append((r, 'pool' in block or 'strided' in block))
        r *= 2
        blocks = []
    return plan


def _pooled_levels(config):
    return sum(1 for _, pooled in _layer_plan(config) if pooled)


def level_capacity(B, N, caps):
    """Rows of every level buffer of B clouds of N points under per-cloud caps (levels 1..): C_0 = B*N,
    C_l = min(C_{l-1}, 64*ceil(B*caps[l-1]/64)).  Plain host code."""
    C = [int(B) * int(N)]
    for c in caps:
        C.append(min(C[-1], 64 * int(math.ceil(int(B) * float(c) / 64.0))))
    return C


def _checked_caps(caps, levels):
    """caps as a tuple of `levels` positive finite numbers (None stays None)."""
    if caps is None:
        return None
    if isinstance(caps, (str, bytes)) or not hasattr(caps, '__len__') or len(caps) != levels:
        raise ValueError('set_level_caps: a sequence of %d per-cloud row caps (levels 1..%d), or None; got %r'
                         % (levels, levels, caps))
    out = []
    for c in caps:
        if isinstance(c, bool) or not isinstance(c, (int, float, np.integer, np.floating)) or not math.isfinite(c) or c <= 0:
            raise ValueError('set_level_caps: every cap is a positive finite number (got %r in %r)' % (c, tuple(caps)))
        out.append(int(c) if float(c).is_integer() else float(c))
    return tuple(out)


def calibrate_level_caps(batches, config=None, margin=1.15):
    """Per-cloud caps for `set_level_caps` from sample batches: the exact-size preprocessing runs over an iterable of
    [B,3,N,1] device batches, and per level the largest total / B seen, times `margin`, rounded up, is returned.  This is
    the one place that waits for the host, once, before training."""
    config = KPConvConfig if config is None else config
    pre = PreprocessorGPU(config)
    worst = None
    for x in batches:
        pts, lengths = _split_clouds(x)
        meta = pre.forward_packed(pts, lengths)
        per = [sum(l) / float(len(lengths)) for l in meta['lengths'][1:]]
        worst = per if worst is None else [max(a, b) for a, b in zip(worst, per)]
    if worst is None:
        raise ValueError('calibrate_level_caps: no batches')
    return tuple(max(1, int(math.ceil(w * float(margin)))) for w in worst)


class LevelCaps:
    """set_level_caps / capacity_report of a module with a `preprocessor` (KPConv_g, KPFCls)."""

    def set_level_caps(self, caps):
        """caps: 4 positive numbers -- the rows PER CLOUD allowed at levels 1..4 -- or None for the exact-size path.
        While caps are set the module is graph_capturable: nothing in its forward or backward waits for the host."""
        caps = _checked_caps(caps, _pooled_levels(self.config))
        self.preprocessor.set_level_caps(caps)
        self.level_caps = caps
        self.graph_capturable = caps is not None

    def capacity_report(self, reset=False):
        """One host read of the capacity record.  {'levels': [{'level', 'capacity' (rows in force, of the last forward's
        batch), 'needed' (most rows any forward needed so far), 'cap' (the per-cloud cap in force), 'cap_needed' (the
        per-cloud cap that would have sufficed for the last batch size)}, ...], 'overflows': forwards in which a level
        overflowed}; reset=True clears the record."""
        return self.preprocessor.capacity_report(reset)


class PreprocessorGPU(nn.Module):
    """Computes the metadata used for KPConv on the device (deterministic: voxels in first-point order)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.level_caps = None          # per-cloud caps of levels 1.. (capacity form), None: exact sizes
        self._record = None             # int32 [ops.KPCONV_RECORD_INTS] on the device: needed rows per level, overflows
        self._shape = None              # (B, N) of the last capacity forward

    def set_level_caps(self, caps):
        self.level_caps = None if caps is None else tuple(caps)
        self._record = self._shape = None

    def _record_on(self, dev):
        if self._record is None or self._record.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('KPConv capacity record: the first forward with level caps must run outside a capture')
            self._record = torch.zeros(ops.KPCONV_RECORD_INTS, dtype=torch.int32, device=dev)
        return self._record

    def capacity_report(self, reset=False):
        if self.level_caps is None:
            raise RuntimeError('capacity_report: no level caps are set (set_level_caps)')
        rec = [0] * ops.KPCONV_RECORD_INTS if self._record is None else self._record.tolist()   # the one host read
        if reset and self._record is not None:
            self._record.zero_()
        B, N = self._shape if self._shape is not None else (1, 0)
        C = level_capacity(B, N, self.level_caps)
        levels = [{'level': l + 1, 'capacity': C[l + 1], 'needed': rec[l], 'cap': self.level_caps[l],
                   'cap_needed': int(math.ceil(rec[l] / float(B)))} for l in range(len(self.level_caps))]
        return {'levels': levels, 'overflows': rec[4]}

    def forward(self, pts: List[torch.Tensor]):
        """pts: list of point clouds XYZ [Ni, 3] (fp32, HIP device)."""
        return self.forward_packed(torch.cat([p.float() for p in pts], 0).contiguous(), [int(p.shape[0]) for p in pts])

    def forward_packed(self, points, lengths):
        """points [sum Ni, 3] packed on the device, lengths: host ints.  One builder for both forms: with level caps every
        level buffer has its static capacity and every count stays on the device; without, the buffers are sliced to their
        totals after the one synchronisation of the forward."""
        ops._need_gpu(points)
        config = self.cfg
        plan = _layer_plan(config)
        limits = config.neighborhood_limits
        dev = points.device
        B, cap = len(lengths), int(max(lengths))
        if cap > ops.KPCONV_MAX_CLOUD:
            raise NotImplementedError('KPConv preprocessing: clouds of at most %d points (got %d)' % (ops.KPCONV_MAX_CLOUD, cap))
        if self.level_caps is not None:
            if len(set(lengths)) != 1:
                raise NotImplementedError('KPConv preprocessing with level caps: clouds of one length (got %r)' % (lengths,))
            C = level_capacity(B, cap, self.level_caps)
            rec = self._record_on(dev)
            self._shape = (B, cap)
            off0 = torch.arange(0, (B + 1) * cap, cap, dtype=torch.int32, device=dev)
        else:
            C = rec = None
            off0 = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32).to(dev, non_blocking=True)
        bufs, offs = [points], [off0]
        for li, (r, pooled) in enumerate(plan):
            if not pooled:
                break
            p, o = ops.kp_grid_subsample(bufs[-1], offs[-1], B, cap, 2 * r / config.conv_radius,
                                         rows=C[li + 1] if C else None, record=rec, level=li)
            bufs.append(p)
            offs.append(o)
        stack = torch.stack(offs)
        lens = None
        if C is None:
            # the one synchronisation of the forward: every level's offsets
            off_host = stack.cpu().numpy().astype(np.int64)
            lens = [list(map(int, np.diff(o))) for o in off_host]
            bufs = [b[:int(o[-1])] for b, o in zip(bufs, off_host)]
        neighbors, pools, upsamples, rev_n, rev_p = [], [], [], [], []
        for li, (r, pooled) in enumerate(plan):
            Ns = bufs[li].shape[0]
            nb = ops.radius_neighbors(bufs[li], offs[li], bufs[li], offs[li], r, limits[li])
            neighbors.append(nb)
            rev_n.append(ops.radius_reverse(nb, offs[li], offs[li], Ns, cap))
            if pooled:
                pl = ops.radius_neighbors(bufs[li + 1], offs[li + 1], bufs[li], offs[li], r, limits[li])
                pools.append(pl)
                rev_p.append(ops.radius_reverse(pl, offs[li + 1], offs[li], Ns, cap))
                upsamples.append(ops.radius_neighbors(bufs[li], offs[li], bufs[li + 1], offs[li + 1], 2 * r, limits[li]))
            else:
                empty = torch.zeros((0, 1), dtype=torch.int32, device=dev)
                pools.append(empty)
                upsamples.append(empty)
                rev_p.append(None)
        return {
            'points': bufs,
            'neighbors': neighbors,
            'pools': pools,
            'upsamples': upsamples,
            'stack_lengths': list((stack[:, 1:] - stack[:, :-1]).to(torch.int64).unbind(0)),
            # this build's additions: device offsets, reverse lists, host lengths (exact sizes only: with level caps
            # nothing may need them), the level capacities (with level caps only)
            'offsets': offs,
            'rev_neighbors': rev_n,
            'rev_pools': rev_p,
            'lengths': lens,
            'capacities': C,
        }


class KPFEncoder(nn.Module):
    def __init__(self, config, increase_channel_when_downsample=True):
        super().__init__()
        octave = 0
        r = config.first_subsampling_dl * config.conv_radius
        in_dim = config.in_feats_dim
        out_dim = config.first_feats_dim
        self.encoder_blocks = nn.ModuleList()
        self.encoder_skip_dims = []
        self.encoder_skips = []
        for block_i, block in enumerate(config.architecture):
            if ('equivariant' in block) and (not out_dim % 3 == 0):
                raise ValueError('Equivariant block but features dimension is not a factor of 3')
            if np.any([tmp in block for tmp in ['pool', 'strided', 'upsample', 'global']]):
                self.encoder_skips.append(block_i)
                self.encoder_skip_dims.append(in_dim)
            if 'upsample' in block:
                break
            self.encoder_blocks.append(block_decider(block, r, in_dim, out_dim, octave, config))
            in_dim = out_dim // 2 if 'simple' in block else out_dim
            if 'pool' in block or 'strided' in block:
                octave += 1
                r *= 2
                if increase_channel_when_downsample:
                    out_dim *= 2
        if 'upsample' not in block:
            self.encoder_skips.append(block_i)
            self.encoder_skip_dims.append(in_dim)
        self.layer_idx = octave

    def forward(self, x, batch):
        """(x, skip_x, mid_fea): mid_fea = the output of block 2, detached (as the reference)."""
        skip_x = []
        mid_fea = None
        for block_i, block_op in enumerate(self.encoder_blocks):
            if block_i in self.encoder_skips:
                skip_x.append(x)
            x = block_op(x, batch)
            if block_i == 2:
                mid_fea = x.detach()
        return x, skip_x, mid_fea


class GlobalAverageBlock(nn.Module):

    def __init__(self):
        super(GlobalAverageBlock, self).__init__()

    def forward(self, x, len):
        """len: the last level's device offsets [B+1] (int32) in this build (the reference: stack lengths)."""
        return global_average(x, len)


def _split_clouds(x):
    """[B,3,N,1] clouds -> (packed points [B*N, 3], host lengths)."""
    B, N = x.shape[0], x.shape[2]
    pts = x.squeeze(-1).permute(0, 2, 1)[:, :, :3].reshape(B * N, 3).contiguous()
    return pts, [N] * B


class KPFCls(LevelCaps, nn.Module):
    """model/KPConv_model.py:60-90.  B = 1 works here (the reference builds an empty cloud list for it)."""

    graph_capturable = False        # level sizes depend on the data, as KPConv_g's: SourceStep runs it eagerly --
    level_caps = None               # unless set_level_caps(caps) fixes the level capacities (then True, on the instance)

    def __init__(self, config=None, increase_channel_when_downsample=True):
        super().__init__()
        self.config = KPConvConfig if config is None else config
        self.preprocessor = PreprocessorGPU(self.config)
        self.encoder = KPFEncoder(self.config)
        self.global_avg_pooling = GlobalAverageBlock()
        self.fc = nn.Sequential(nn.Linear(1024, 256), nn.ReLU(), nn.Linear(256, 64), nn.ReLU(),
                                nn.Linear(64, self.config.num_class))
        self.deform_fitting_power = self.config.deform_fitting_power

    def forward(self, x):
        pts, lengths = _split_clouds(x)
        kpconv_meta = self.preprocessor.forward_packed(pts, lengths)
        feats0 = kpconv_meta["points"][0][:, 0:1]
        feats = self.encoder(feats0, kpconv_meta)
        feats_avg = self.global_avg_pooling(feats[0], kpconv_meta["offsets"][-1])
        return self.fc(feats_avg)


def p2p_fitting_regularizer(net, deform_fitting_power=1):
    """model/KPConv_model.py:282-315: the deformable kernels' fitting and repulsion terms -- 0 for rigid kernels, the
    only ones built."""
    for m in net:
        if hasattr(m, "KPConv") and m.KPConv.deformable:
            raise NotImplementedError('p2p_fitting_regularizer: deformable KPConv is not built')
    return 0


__all__ = ['level_capacity', 'calibrate_level_caps', 'KPConvConfig', 'PreprocessorGPU', 'KPFEncoder', 'GlobalAverageBlock', 'KPFCls', 'p2p_fitting_regularizer',
           'UnaryBlock']
