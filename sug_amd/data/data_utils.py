"""data/data_utils.py on the device: each function is sug_prepare_batch with the other stages switched off.

A cloud is a device tensor [P, C>=3] (or a batch [B, P, C]); only xyz is used, the result is fp32 [P', 3] (or
[B, P', 3]).  The random functions draw in the kernel from (module seed, call counter): `manual_seed(s)` restarts the
sequence, every call advances it, so two calls never share a draw and a run is reproducible.  Each of them also takes
the draw itself (`angle=`, `noise=`, `point_idx=`) in place of the generator.
"""
import torch

from .. import ops

_state = {'seed': 0, 'calls': 0}


def manual_seed(seed):
    """Restart the generator of rotation_point_cloud / jitter_point_cloud / pc_augment / random_sample_pc."""
    _state['seed'], _state['calls'] = int(seed), 0


def _batch(pc):
    ops._need_gpu(pc)
    single = pc.dim() == 2
    x = pc.unsqueeze(0) if single else pc
    if x.dim() != 3 or x.shape[2] < 3:
        raise ValueError('expected a cloud [P, C>=3] or a batch [B, P, C>=3], got %s' % (tuple(pc.shape),))
    return x[:, :, :3].to(torch.float32).contiguous(), single


def _run(pc, num_points=None, stages=0, pre_matrix=None, angle=None, noise=None, point_idx=None, sigma=0.01, clip=0.05):
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
    counter = None
    drawn = ((stages & ops.PREP_ROTATE_Z) and angles is None) or ((stages & ops.PREP_JITTER) and noise is None) or \
        ((P > N or (stages & ops.PREP_SHUFFLE)) and sel is None)
    if drawn:
        counter = torch.tensor([_state['calls']], dtype=torch.int64, device=dev)
        _state['calls'] += 1
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


def pc_augment(pc, angle=None, noise=None):
    """rotation_point_cloud, then jitter_point_cloud (data/data_utils.py:169-175)."""
    return _run(pc, stages=ops.PREP_ROTATE_Z | ops.PREP_JITTER, angle=angle, noise=noise)


def random_sample_pc(pts, num_points, point_idx=None):
    """The first num_points of a random permutation of the points (data/data_utils.py:178-182); `point_idx`
    [num_points]: the kept indices in order."""
    P = pts.shape[-2]
    if num_points > P:
        raise ValueError('random_sample_pc: num_points=%d > %d points' % (num_points, P))
    return _run(pts, num_points=num_points, stages=ops.PREP_SHUFFLE, point_idx=point_idx)
