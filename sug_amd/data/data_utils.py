"""data/data_utils.py on the device: each function is sug_prepare_batch with the other stages switched off.

A cloud is a device tensor [P, C>=3] (or a batch [B, P, C]); only xyz is used, the result is fp32 [P', 3] (or
[B, P', 3]).  The random functions draw in the kernel from (module seed, call counter): `manual_seed(s)` restarts the
sequence, every call advances it, so two calls never share a draw and a run is reproducible.  Each of them also takes
the draw itself (`angle=`, `noise=`, `point_idx=`, `scales=`, `normals=`, `shifts=`) in place of the generator.
shift_point_cloud / random_scale_point_cloud / rotate_perturbation_point_cloud run sug_prepare_batch_aug.
"""
import torch

from .. import ops

_state = {'seed': 0, 'calls': 0}


def manual_seed(seed):
    """Restart the generator of the random functions of this module."""
    _state['seed'], _state['calls'] = int(seed), 0


def _batch(pc):
    ops._need_gpu(pc)
    single = pc.dim() == 2
    x = pc.unsqueeze(0) if single else pc
    if x.dim() != 3 or x.shape[2] < 3:
        raise ValueError('expected a cloud [P, C>=3] or a batch [B, P, C>=3], got %s' % (tuple(pc.shape),))
    return x[:, :, :3].to(torch.float32).contiguous(), single


def _per_cloud(t, B, width, dev):
    """A supplied per-cloud draw: one value (or one `width`-vector) for every cloud, or one per cloud."""
    t = torch.as_tensor(t, dtype=torch.float32, device=dev).reshape(-1, width)
    return (t.expand(B, width) if t.shape[0] == 1 else t).reshape((B, width) if width > 1 else (B,)).contiguous()


def _run(pc, num_points=None, stages=0, pre_matrix=None, angle=None, noise=None, point_idx=None, sigma=0.01, clip=0.05,
         scales=None, normals=None, shifts=None, **params):
    x, single = _batch(pc)
    B, P, _ = x.shape
    dev = x.device
    N = P if num_points is None else int(num_points)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    angles = sel = None
    if angle is not None:
        angles = torch.as_tensor(angle, dtype=torch.float32, device=dev).reshape(-1).expand(B).contiguous()
    if noise is not None:
        noise = noise.to(device=dev, dtype=torch.float32).reshape(B, P, 3).contiguous()
    if point_idx is not None:
        sel = point_idx.to(device=dev, dtype=torch.int32).reshape(B, N).contiguous()
    if scales is not None:
        scales = _per_cloud(scales, B, 1, dev)
    if normals is not None:
        normals = _per_cloud(normals, B, 3, dev)
    if shifts is not None:
        shifts = _per_cloud(shifts, B, 3, dev)
    counter = None
    drawn = ((stages & ops.PREP_ROTATE_Z) and angles is None) or ((stages & ops.PREP_JITTER) and noise is None) or \
        ((P > N or (stages & ops.PREP_SHUFFLE)) and sel is None) or ((stages & ops.PREP_SCALE) and scales is None) or \
        ((stages & ops.PREP_PERTURB) and normals is None) or ((stages & ops.PREP_SHIFT) and shifts is None)
    if drawn:
        counter = torch.tensor([_state['calls']], dtype=torch.int64, device=dev)
        _state['calls'] += 1
    if stages & (ops.PREP_SCALE | ops.PREP_PERTURB | ops.PREP_SHIFT):
        out = ops.prepare_batch_aug(x, idx, N, False, False, angles=angles, noise=noise, sel=sel, scales=scales, perturb=normals,
                                    shifts=shifts, seed=_state['seed'], counter=counter, sigma=sigma, clip=clip, stages=stages,
                                    pre_matrix=pre_matrix, **params)
    else:
        out = ops.prepare_batch(x, idx, N, False, False, angles=angles, noise=noise, sel=sel, seed=_state['seed'],
                                counter=counter, sigma=sigma, clip=clip, stages=stages, pre_matrix=pre_matrix)
    out = out.transpose(1, 2)                  # [B, N, 3], the reference's point-major layout
    return out[0] if single else out


def normal_pc(pc):
    """Subtract the mean, divide by the largest norm (data/data_utils.py:5-15)."""
    return _run(pc, stages=ops.PREP_NORMALIZE)


def rotate_shape(x, axis, angle):
    """x.dot(R_axis(angle)) (data/data_utils.py:38-56)."""
    return _run(x, pre_matrix=ops.rotation_matrix(axis, angle))


def rotation_point_cloud(pc, angle=None):
    """One random rotation about z per cloud (data/data_utils.py:59-82)."""
    return _run(pc, stages=ops.PREP_ROTATE_Z, angle=angle)


def jitter_point_cloud(pc, sigma=0.01, clip=0.05, noise=None):
    """pc + clip(sigma * randn, -clip, clip) (data/data_utils.py:106-116); `noise` [P, 3]: the standard-normal draws."""
    return _run(pc, stages=ops.PREP_JITTER, noise=noise, sigma=sigma, clip=clip)


def rotate_point_cloud_by_angle(pc, rotation_angle):
    """One rotation about y by the given angle (data/data_utils.py:85-103): rotate_shape's 'y' matrix."""
    return _run(pc, pre_matrix=ops.rotation_matrix('y', rotation_angle))


def shift_point_cloud(pc, shift_range=0.1, shifts=None):
    """pc + t, one t uniform in [-shift_range, shift_range)^3 per cloud (data/data_utils.py:119-129); `shifts` [3] or
    [B, 3]: the vector itself.  Returns a new tensor -- the reference adds to its argument in place."""
    return _run(pc, stages=ops.PREP_SHIFT, shifts=shifts, shift_range=shift_range)


def random_scale_point_cloud(pc, scale_low=0.8, scale_high=1.25, scales=None):
    """pc * s, one s uniform in [scale_low, scale_high) per cloud (data/data_utils.py:132-142); `scales` [1] or [B]: the
    factor itself.  Returns a new tensor -- the reference scales its argument in place."""
    return _run(pc, stages=ops.PREP_SCALE, scales=scales, scale_low=scale_low, scale_high=scale_high)


def rotate_perturbation_point_cloud(pc, angle_sigma=0.06, angle_clip=0.18, normals=None):
    """pc . (Rz Ry Rx) of three small angles clip(angle_sigma * randn(3), +-angle_clip) per cloud (data/data_utils.py:145-166);
    `normals` [3] or [B, 3]: the standard-normal draws."""
    return _run(pc, stages=ops.PREP_PERTURB, normals=normals, angle_sigma=angle_sigma, angle_clip=angle_clip)


def pc_augment(pc, angle=None, noise=None, scale=False, perturb=False, shift=False, scales=None, normals=None, shifts=None):
    """rotation_point_cloud, then jitter_point_cloud (data/data_utils.py:169-175); `scale`, `perturb`, `shift` switch on
    the three lines the reference has commented out, in its line order and with the functions' default parameters."""
    stages = ops.PREP_ROTATE_Z | ops.PREP_JITTER | (ops.PREP_SCALE if scale else 0) | (ops.PREP_PERTURB if perturb else 0) | \
        (ops.PREP_SHIFT if shift else 0)
    return _run(pc, stages=stages, angle=angle, noise=noise, scales=scales, normals=normals, shifts=shifts)


def random_sample_pc(pts, num_points, point_idx=None):
    """The first num_points of a random permutation of the points (data/data_utils.py:178-182); `point_idx`
    [num_points]: the kept indices in order."""
    P = pts.shape[-2]
    if num_points > P:
        raise ValueError('random_sample_pc: num_points=%d > %d points' % (num_points, P))
    return _run(pts, num_points=num_points, stages=ops.PREP_SHUFFLE, point_idx=point_idx)


def fps(points, n_samples):
    """Farthest-point sampling from point 0, ties to the lowest index (data/data_utils.py:185-229) -> the sampled points
    [n_samples, 3] (or [B, n_samples, 3]): ops.fps as dataset_splitter.process_pts calls it."""
    x, single = _batch(points)
    if not 1 <= n_samples <= x.shape[1]:
        raise ValueError('fps: n_samples=%d of %d points' % (n_samples, x.shape[1]))
    idx = ops.fps(x, int(n_samples), torch.zeros(x.shape[0], dtype=torch.int32, device=x.device))
    out = torch.gather(x, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
    return out[0] if single else out


def farthest_point_sample(xyz, npoint):
    """xyz [B, C, N] -> (centroids int64 [B, npoint], centroids_vals [B, C, npoint]) (data/data_utils.py:258-282).  The
    start points come from torch.randint on the host generator, the reference's one draw; the distances use xyz's first
    three channels (the FPS kernel's), so C > 3 differs from the reference, which sums over all C."""
    ops._need_gpu(xyz)
    if xyz.dim() != 3 or xyz.shape[1] < 3:
        raise ValueError('farthest_point_sample: expected [B, C>=3, N], got %s' % (tuple(xyz.shape),))
    B, C, N = xyz.shape
    farthest = torch.randint(0, N, (B,), dtype=torch.long)
    rows = xyz[:, :3].transpose(1, 2).to(torch.float32).contiguous()
    centroids = ops.fps(rows, int(npoint), farthest).long()
    return centroids, torch.gather(xyz, 2, centroids.unsqueeze(1).expand(-1, C, -1))
