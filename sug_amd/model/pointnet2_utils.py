"""Point-set operators in the [B,N,C] layout and the PointNet++ modules -- set abstraction, multi-scale grouping and
feature propagation (mirror of the reference's model/pointnet2_utils.py:19-320), over the HIP kernels."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .model_utils import _bn_rows


def square_distance(src, dst):
    """model/pointnet2_utils.py:19-38 ([B,N,C] x [B,M,C] -> [B,N,M]); API parity only."""
    B, N, _ = src.shape
    M = dst.shape[1]
    d = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    d = d + torch.sum(src ** 2, -1).view(B, N, 1)
    d = d + torch.sum(dst ** 2, -1).view(B, 1, M)
    return d


def index_points(points, idx):
    """model/pointnet2_utils.py:41-57. points [B,N,C], idx [B,S(,K)] -> [B,S(,K),C]."""
    return ops.gather_rows(points, idx)


def farthest_point_sample(xyz, npoint):
    """model/pointnet2_utils.py:60-81. xyz [B,N,3] -> [B,npoint] int64 (CPU-generator start, :72)."""
    B, N, _ = xyz.shape
    start = ops.draw_start(B, N)
    return ops.fps(xyz, npoint, start).long()


def query_ball_point(radius, nsample, xyz, new_xyz):
    """model/pointnet2_utils.py:84-104. xyz [B,N,3], new_xyz [B,S,3] -> [B,S,nsample] int64."""
    return ops.ball_query(xyz, new_xyz, radius, nsample).long()


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False):
    """model/pointnet2_utils.py:107-135 -> new_xyz [B,S,3], new_points [B,S,nsample,3+D]."""
    B, N, C = xyz.shape
    start = ops.draw_start(B, N)
    fps_idx = ops.fps(xyz, npoint, start)
    new_xyz = ops.gather_rows(xyz, fps_idx)
    idx = ops.ball_query(xyz, new_xyz, radius, nsample)
    grouped_xyz = ops.gather_rows(xyz, idx)
    new_points = grouped_xyz - new_xyz.view(B, npoint, 1, C)
    if points is not None:
        new_points = torch.cat([new_points, ops.gather_rows(points, idx)], dim=-1)
    if returnfps:
        return new_xyz, new_points, grouped_xyz, fps_idx.long()
    return new_xyz, new_points


def sample_and_group_idx(npoint, radius, nsample, xyz):
    """The index half of sample_and_group (model/pointnet2_utils.py:107-124): same FPS start draw and kernels,
    -> new_xyz [B,S,3], idx [B,S,nsample] int32; the grouped tensor itself is not formed."""
    B, N, _ = xyz.shape
    plan = ops.CTX.geometry_plan
    if plan:
        new_xyz, idx = plan.pop(0)              # computed up front for this pass (Pointnet2_g.plan_geometry)
        if new_xyz.shape != (B, npoint, 3) or idx.shape != (B, npoint, nsample):
            raise RuntimeError('geometry plan does not match the encoder: %s / %s for (%d, %d, %d)' % (
                tuple(new_xyz.shape), tuple(idx.shape), B, npoint, nsample))
        return new_xyz, idx
    start = ops.draw_start(B, N)
    fps_idx = ops.fps(xyz, npoint, start)
    new_xyz = ops.gather_rows(xyz, fps_idx)
    return new_xyz, ops.ball_query(xyz, new_xyz, radius, nsample)


def sample_and_group_all(xyz, points):
    """model/pointnet2_utils.py:138-155."""
    B, N, C = xyz.shape
    new_xyz = torch.zeros(B, 1, C, device=xyz.device)
    grouped = xyz.view(B, 1, N, C)
    if points is not None:
        grouped = torch.cat([grouped, points.view(B, 1, N, -1)], dim=-1)
    return new_xyz, grouped


class PointNetSetAbstraction(nn.Module):
    """model/pointnet2_utils.py:158-207: FPS -> ball query -> group -> 1x1 conv/BN/ReLU stack ->
    max over the group.  Parameters are named as in the reference (mlp_convs.i, mlp_bns.i)."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all, adapt=False):
        super(PointNetSetAbstraction, self).__init__()
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        self.adapt = adapt
        last = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last = out_channel
        self.group_all = group_all

    def takes_index_path(self):
        """True if rows() runs its first MLP layer on the neighbour lists (sample_and_group_idx -- the only consumer of an
        ops.CTX.geometry_plan) instead of forming the grouped tensor."""
        return (not self.group_all) and len(self.mlp_convs) > 1 and \
            ops.sa_first_layer_supported(self.mlp_convs[0].out_channels)

    def rows(self, xyz, points, adapt=False, tail_grad=True):
        """xyz [B,N,3], points [B,N,D] or None -> new_xyz [B,S,3], feats [B,S,D'](, node [B,S,D1]).
        tail_grad=False (with adapt): the layers behind the one the node features come from run without
        autograd (their output is discarded by the caller; BatchNorm buffers are still updated)."""
        first = 0
        if self.group_all:
            new_xyz, g = sample_and_group_all(xyz, points)
        elif self.takes_index_path():
            # first layer on the neighbour lists: W.[x_j - c_s ; f_j] + b = P[j] - Q[s], P per point, Q per centroid
            # (the grouped [B,S,ns,3+D] tensor and the pre-activation tensor are never formed)
            new_xyz, idx = sample_and_group_idx(self.npoint, self.radius, self.nsample, xyz)
            conv = self.mlp_convs[0]
            w = conv.weight.view(conv.weight.shape[0], -1)
            if ops.SA_FIRST_GEO and xyz.shape[-1] == 3:
                # coordinate part from the difference the reference forms: y = Pf[j] + b + Wx.(x_j - c_s) (sug_sa_first_geo_*);
                # Px and Q only route the gradients of Wx and b (their values are not read by the kernel)
                wx = w[:, :3].contiguous()
                Px = ops.linear_rows(xyz, wx)
                Pf = None if points is None else ops.linear_rows(points, w[:, 3:].contiguous())
                Q = ops.sub_row_bias(ops.linear_rows(new_xyz, wx), conv.bias)
                g = ops.sa_first_layer_geo(Pf, Px, Q, idx, xyz, new_xyz, wx, conv.bias, self.mlp_bns[0])
            else:
                P = ops.linear_rows(xyz if points is None else torch.cat((xyz, points), dim=-1), w)
                Q = ops.sub_row_bias(ops.linear_rows(new_xyz, w[:, :3]), conv.bias)
                g = ops.sa_first_layer(P, Q, idx, self.mlp_bns[0])
            first = 1
        else:
            new_xyz, g = sample_and_group(self.npoint, self.radius, self.nsample, xyz, points)
        node = None
        last = len(self.mlp_convs) - 1
        out = None
        for i, conv in enumerate(self.mlp_convs):                      # g: [B,S,ns,C] rows
            if i < first:
                continue
            w = conv.weight.view(conv.weight.shape[0], -1)
            if i == last - 1 and ops.SA_MID_FUSED and g.is_cuda and self.mlp_bns[i].training == self.mlp_bns[last].training and \
                    ops.pointmlp_max_supported(w.shape[0], self.mlp_convs[last].out_channels, g.shape[2]):
                # middle layer + last layer: the middle layer's BatchNorm + ReLU is applied inside the fused last-layer
                # kernel (ops.bn_act_pointmlp_max): no separate pass over [B,S,ns,C], z written once and only if needed
                tail_on = tail_grad or not adapt           # (node pass: the last layer runs for its BatchNorm buffers only)
                y1 = ops.linear_rows(g, w, conv.bias)
                cl = self.mlp_convs[last]
                out, z = ops.bn_act_pointmlp_max(y1, self.mlp_bns[i], 0.0, cl.weight.view(cl.weight.shape[0], -1), cl.bias,
                                                 self.mlp_bns[last], 0.0, g.shape[2], want_z=(adapt and i == 1),
                                                 last_grad=tail_on)
                out = out.view(g.shape[0], g.shape[1], -1)
                if adapt and i == 1:
                    node = z
                break
            with torch.set_grad_enabled(torch.is_grad_enabled() and (tail_grad or not adapt or i <= 1)):
                if i == last and ops.pointmlp_max_supported(g.shape[-1], w.shape[0], g.shape[2]):
                    # last layer + max over the group in one kernel: [B,S,ns,C'] is never written
                    out = ops.pointmlp_max(g, w, conv.bias, self.mlp_bns[i], 0.0, g.shape[2]).view(g.shape[0], g.shape[1], -1)
                    break
                g = ops.bn_act_rows(ops.linear_rows(g, w, conv.bias), self.mlp_bns[i], 0.0)
            if adapt and i == 1:
                node = g
        if out is None:
            out = torch.max(g, dim=2)[0]
        if adapt:
            return new_xyz, out, torch.max(node, dim=2)[0]
        return new_xyz, out

    def forward(self, xyz, points, adapt=False):
        """Reference layout: xyz [B,3,N], points [B,D,N] -> new_xyz [B,3,S], new_points [B,D',S]."""
        r = self.rows(xyz.permute(0, 2, 1).contiguous(),
                      None if points is None else points.permute(0, 2, 1).contiguous(), adapt)
        return tuple(t.permute(0, 2, 1) for t in r)


def _msg_scale_rows(convs, bns, xyz, points, new_xyz, idx):
    """One scale of multi-scale grouping (model/pointnet2_utils.py:249-262) on rows: the (1x1 conv, BN, ReLU) stack over the
    groups of `idx` [B,S,K] and the max over each group -> [B,S,D'].  Channel order of a group is [features, xyz - centre]
    (:253): the coordinate columns of the first layer are its LAST three.  What PointNetSetAbstraction.rows does per layer:
    the first one on the neighbour lists where its width and the list size allow (no grouped [B,S,K,3+D] tensor), the last one fused
    with the max where the widths allow, the general rows kernels otherwise."""
    B, S, K = idx.shape
    conv = convs[0]
    w = conv.weight.view(conv.weight.shape[0], -1)
    last = len(convs) - 1
    first = 0
    if last > 0 and ops.sa_first_layer_supported(w.shape[0]) and ops.reverse_lists_fit(B, xyz.shape[1], S * K):
        # y = Wf.f_j + b + Wx.(x_j - c_s), the coordinate part from the difference the reference forms (sug_sa_first_geo_*): at
        # the small radii of the first scales P[j] - Q[s] cancels, and BatchNorm divides the residue by a small deviation.
        # Px and Q only route the gradients of Wx and b (their values are not read by the kernel)
        wx = w[:, -3:].contiguous()
        Px = ops.linear_rows(xyz, wx)
        Pf = None if points is None else ops.linear_rows(points, w[:, :-3].contiguous())
        Q = ops.sub_row_bias(ops.linear_rows(new_xyz, wx), conv.bias)
        g = ops.sa_first_layer_geo(Pf, Px, Q, idx, xyz, new_xyz, wx, conv.bias, bns[0])
        first = 1
    else:
        g = ops.gather_rows(xyz, idx) - new_xyz.view(B, S, 1, 3)
        if points is not None:
            g = torch.cat([ops.gather_rows(points, idx), g], dim=-1)
    for i in range(first, last + 1):                                  # g: [B,S,K,C] rows
        conv = convs[i]
        w = conv.weight.view(conv.weight.shape[0], -1)
        if i == last - 1 and ops.SA_MID_FUSED and bns[i].training == bns[last].training and \
                ops.pointmlp_max_supported(w.shape[0], convs[last].out_channels, K):
            # middle layer's BatchNorm + ReLU inside the fused last-layer + max kernel
            cl = convs[last]
            out, _ = ops.bn_act_pointmlp_max(ops.linear_rows(g, w, conv.bias), bns[i], 0.0, cl.weight.view(cl.weight.shape[0], -1),
                                             cl.bias, bns[last], 0.0, K)
            return out.view(B, S, -1)
        if i == last and ops.pointmlp_max_supported(g.shape[-1], w.shape[0], K):
            return ops.pointmlp_max(g, w, conv.bias, bns[i], 0.0, K).view(B, S, -1)
        g = ops.bn_act_rows(ops.linear_rows(g, w, conv.bias), bns[i], 0.0)
    return torch.max(g, dim=2)[0]


class PointNetSetAbstractionMsg(nn.Module):
    """model/pointnet2_utils.py:210-267: FPS once, then per radius ball query -> group -> 1x1 conv/BN/ReLU stack -> max over
    the group, the scales' features concatenated.  The lists of all radii come from one pass over the distances
    (ops.ball_query_multi).  Parameters are named as in the reference (conv_blocks.i.j, bn_blocks.i.j)."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super(PointNetSetAbstractionMsg, self).__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for widths in mlp_list:                                        # one (conv, BN) stack per radius; input [features, xyz - centre]
            stack = [in_channel + 3] + list(widths)
            self.conv_blocks.append(nn.ModuleList(nn.Conv2d(a, b, 1) for a, b in zip(stack[:-1], stack[1:])))
            self.bn_blocks.append(nn.ModuleList(nn.BatchNorm2d(b) for b in stack[1:]))

    def group_indices(self, xyz):
        """xyz [B,N,3] -> new_xyz [B,S,3], fps_idx [B,S] int32, [idx_i [B,S,K_i] int32]: ONE start draw from the CPU
        generator (:244), the lists of up to four radii per launch."""
        B, N, _ = xyz.shape
        fps_idx = ops.fps(xyz, self.npoint, ops.draw_start(B, N))
        new_xyz = ops.gather_rows(xyz, fps_idx)
        lists = []
        for r0 in range(0, len(self.radius_list), 4):
            lists += ops.ball_query_multi(xyz, new_xyz, list(self.radius_list[r0:r0 + 4]), list(self.nsample_list[r0:r0 + 4]))
        return new_xyz, fps_idx, lists

    def rows(self, xyz, points):
        """xyz [B,N,3], points [B,N,D] or None -> new_xyz [B,S,3], feats [B,S,sum D'_i]."""
        new_xyz, _, lists = self.group_indices(xyz.detach())
        parts = [_msg_scale_rows(self.conv_blocks[i], self.bn_blocks[i], xyz, points, new_xyz, idx) for i, idx in enumerate(lists)]
        if len(parts) == 1:
            return new_xyz, parts[0]
        B, S = parts[0].shape[:2]
        buf = torch.empty(B, S, sum(p.shape[-1] for p in parts), dtype=torch.float32, device=xyz.device)
        return new_xyz, ops.assemble_rows(buf, parts)               # each scale lands in its column slice

    def forward(self, xyz, points):
        """Reference layout: xyz [B,3,N], points [B,D,N] or None -> new_xyz [B,3,S], new_points_concat [B,sum D'_i,S]."""
        r = self.rows(xyz.permute(0, 2, 1).contiguous(), None if points is None else points.permute(0, 2, 1).contiguous())
        return tuple(t.permute(0, 2, 1) for t in r)


class PointNetFeaturePropagation(nn.Module):
    """model/pointnet2_utils.py:270-320: 3-NN inverse-distance interpolation of the coarse level's features onto the dense
    level (ops.fp_interp: expanded-form distances, `1 / (d + 1e-8)` weights), concatenated behind points1, then the
    (1x1 conv, BN, ReLU) stack on rows.  Parameters are named as in the reference (mlp_convs.i, mlp_bns.i).  The coordinates
    are data: no gradient flows to them."""
    DIRECT = False                    # distance form of the 3-NN selection (PTran_utils: the direct form)

    def __init__(self, in_channel, mlp):
        super(PointNetFeaturePropagation, self).__init__()
        stack = [in_channel] + list(mlp)
        self.mlp_convs = nn.ModuleList(nn.Conv1d(a, b, 1) for a, b in zip(stack[:-1], stack[1:]))
        self.mlp_bns = nn.ModuleList(nn.BatchNorm1d(b) for b in stack[1:])

    def rows(self, xyz1, xyz2, points1, points2):
        """xyz1 [B,N,3], xyz2 [B,S,3], points1 [B,N,D1] or None, points2 [B,S,D2] -> [B,N,D']."""
        g = ops.fp_interp(xyz1, xyz2, points1, points2, direct=self.DIRECT)
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            g = ops.bn_act_rows(ops.linear_rows(g, conv.weight.view(conv.weight.shape[0], -1), conv.bias), bn, 0.0)
        return g

    def forward(self, xyz1, xyz2, points1, points2):
        """Reference layout: xyz1 [B,C,N], xyz2 [B,C,S], points1 [B,D1,N] or None, points2 [B,D2,S] -> [B,D',N]."""
        return self.rows(xyz1.permute(0, 2, 1).contiguous(), xyz2.permute(0, 2, 1).contiguous(),
                         None if points1 is None else points1.permute(0, 2, 1).contiguous(),
                         points2.permute(0, 2, 1).contiguous()).permute(0, 2, 1)
