#!/usr/bin/env python3
"""Generate tests/golden/kpconv.npz by RUNNING THE REFERENCE's KPConv backbone (build container only, CPU).

Usage (from the repo root, ~1 min):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_kpconv_goldens.py

The reference's KPConv preprocessing calls two third-party operations that are not installed here; small stand-ins,
written for this generator, are registered in sys.modules.  They implement the assumptions the build restates
 -- parity of these two operations is therefore unpinned, as Chamfer's is:
  * pytorch3d.ops.ball_query: per query, the supports of its cloud scanned in index order, the first K with
    d^2 < r^2 kept (d^2 = (s-q)_x^2 + (s-q)_y^2 + (s-q)_z^2 in fp32, left to right; r^2 = fp32(r) * fp32(r)), -1 after;
  * MinkowskiEngine UNWEIGHTED_AVERAGE quantisation: key = floor of the reference's own p / dl (fp32 true division),
    voxels per cloud in order of their first point, the voxel point = fp32 sum in point order / count.
The reference runs with its working directory at model/, so that load_kernels finds its kernel disposition; the
kernel points it draws (numpy-seeded) are stored, every other parameter comes from oracle.ref_cpu.fill_params.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('SUG_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

B, N, SEED = 4, 1024, 7


# ----------------------------------------------------------------------------------------------- stand-ins
class _AttrDict(dict):
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def _ball_query(p1, p2, lengths1=None, lengths2=None, K=50, radius=0.1, return_nn=False):
    Bq, P1 = p1.shape[:2]
    r2 = np.float32(radius) * np.float32(radius)
    idx = torch.full((Bq, P1, K), -1, dtype=torch.int64)
    for b in range(Bq):
        n1, n2 = int(lengths1[b]), int(lengths2[b])
        q, s = p1[b, :n1].float(), p2[b, :n2].float()
        d = s.unsqueeze(0) - q.unsqueeze(1)                                     # [n1, n2, 3], fp32 (s - q)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        hit = d2 < torch.tensor(r2)
        rank = hit.long().cumsum(1) - 1
        keep = hit & (rank < K)
        qi, si = keep.nonzero(as_tuple=True)
        idx[b, qi, rank[qi, si]] = si
    return types.SimpleNamespace(idx=idx)


def _packed_to_padded(x, first_idx, max_size):
    Bp = first_idx.shape[0]
    out = torch.zeros(Bp, max_size, x.shape[1], dtype=x.dtype)
    bounds = list(first_idx.tolist()) + [x.shape[0]]
    for b in range(Bp):
        seg = x[bounds[b]:bounds[b + 1]]
        out[b, :seg.shape[0]] = seg
    return out


class _SparseTensor:
    def __init__(self, features, coordinates, quantization_mode=None):
        coords = coordinates                                                   # list of [Ni, 3] (p / dl)
        self.decomposed_features = []
        i0 = 0
        for c in coords:
            keys = torch.floor(c).to(torch.int64).tolist()
            pts = features[i0:i0 + len(keys)].float().numpy()
            i0 += len(keys)
            order, acc = [], {}
            for j, k in enumerate(map(tuple, keys)):
                if k not in acc:
                    acc[k] = [np.float32(0), np.float32(0), np.float32(0), 0]
                    order.append(k)
                a = acc[k]
                for ax in range(3):
                    a[ax] = np.float32(a[ax] + pts[j, ax])
                a[3] += 1
            mean = np.array([[acc[k][ax] / np.float32(acc[k][3]) for ax in range(3)] for k in order], dtype=np.float32)
            self.decomposed_features.append(torch.from_numpy(mean))
        self.features = torch.cat(self.decomposed_features, 0)


def _install_standins():
    me = types.ModuleType('MinkowskiEngine')
    me.utils = types.SimpleNamespace(batched_coordinates=lambda coords, device=None: list(coords))
    me.SparseTensor = _SparseTensor
    me.SparseTensorQuantizationMode = types.SimpleNamespace(UNWEIGHTED_AVERAGE='unweighted_average')
    sys.modules['MinkowskiEngine'] = me
    p3 = types.ModuleType('pytorch3d')
    p3o = types.ModuleType('pytorch3d.ops')
    p3o.ball_query = _ball_query
    p3o.packed_to_padded = _packed_to_padded
    p3.ops = p3o
    sys.modules['pytorch3d'] = p3
    sys.modules['pytorch3d.ops'] = p3o
    ed = types.ModuleType('easydict')
    ed.EasyDict = _AttrDict
    sys.modules['easydict'] = ed
    for name in ('tkinter', 'turtle', 'chamfer_distance', 'h5py', 'tensorboardX'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['turtle'].distance = None
    sys.modules['chamfer_distance'].ChamferDistance = None
    sys.modules['tensorboardX'].SummaryWriter = object


# ----------------------------------------------------------------------------------------------- inputs
def kpconv_clouds(Bc, Nc, seed):
    """Gaussian blobs and sphere shells, each centred and scaled into the unit sphere: [B, 3, N, 1]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(Bc):
        p = torch.randn(Nc, 3, generator=g)
        if b % 2:
            p = p / p.norm(dim=1, keepdim=True) * (1 + 0.05 * torch.randn(Nc, 1, generator=g))
        p = p * torch.tensor([1.0, 0.7, 0.5])
        p = p - p.mean(0, keepdim=True)
        p = p / p.norm(dim=1).max()
        out.append(p)
    return torch.stack(out).permute(0, 2, 1).unsqueeze(-1).contiguous()


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int64)).tobytes()).hexdigest()


def loss_of(outs, g):
    """The fixed scalar loss of the gradient fixture: fixed random projections of logits, semantic feature, node."""
    y1, y2, f1, f2, ns = outs
    tot = 0
    for i, t in enumerate((y1, y2, f1, ns)):
        r = torch.randn(t.shape, generator=torch.Generator().manual_seed(100 + i), dtype=torch.float64).to(t.dtype)
        tot = tot + (t * r).sum()
    return tot


SMALL_GRADS = ('g.encoder.encoder_blocks.0.KPConv.weights', 'g.encoder.encoder_blocks.1.unary1.mlp.weight',
               'c1.mlp3.weight', 'c1.mlp3.bias', 'attention_s.conv_du.2.bias')


def main():
    _install_standins()
    from oracle import ref_cpu as O
    cwd = os.getcwd()
    os.chdir(os.path.join(REF, 'model'))
    try:
        import model.Model as r_M
        import model.KPConv_model as r_K
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        net = r_M.Net_MDA('KPConv')
        np.random.seed(SEED + 1)
        cls = r_K.KPFCls()
    finally:
        os.chdir(cwd)
    torch.set_num_threads(8)
    out = {}
    for tag, mdl in (('net', net), ('cls', cls)):
        sd = mdl.state_dict()
        kp_keys = [k for k in sd if k.endswith('kernel_points')]
        kps = {k: sd[k].clone() for k in kp_keys}
        filled = O.fill_params({k: tuple(v.shape) for k, v in sd.items()}, SEED)
        filled.update(kps)
        mdl.load_state_dict(filled)
        out[tag + '_keys'] = np.array(list(sd.keys()))
        out[tag + '_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
        out[tag + '_kp_keys'] = np.array(kp_keys)
        out[tag + '_kp'] = np.stack([kps[k].numpy() for k in kp_keys])
    x = kpconv_clouds(B, N, SEED)
    out['x'] = x.numpy()
    net.train()
    cls.train()

    # preprocessing pyramid
    xl = [x.squeeze(-1).permute(0, 2, 1)[i] for i in range(B)]
    meta = net.g.preprocessor(xl)
    L = len(meta['points'])
    out['levels'] = np.array(L)
    for l in range(L):
        out['lengths_%d' % l] = meta['stack_lengths'][l].numpy()
        out['points_%d' % l] = meta['points'][l].numpy()
        out['neighbors_sha_%d' % l] = np.array(sha(meta['neighbors'][l]))
        if l < L - 1:
            out['pools_sha_%d' % l] = np.array(sha(meta['pools'][l]))
            out['upsamples_sha_%d' % l] = np.array(sha(meta['upsamples'][l]))
    print('level lengths', [m.tolist() for m in meta['stack_lengths']])

    # Net_MDA in every mode (train mode; CALayer's BatchNorm1d uses batch statistics)
    with torch.no_grad():
        y1, y2 = net(x)
        out['y1'], out['y2'] = y1.numpy(), y2.numpy()
        r = net(x, semantic_adaption=True)
        out['sem_y1'], out['sem_y2'], out['sem_f1'], out['sem_f2'] = [t.numpy() for t in r]
        out['node_s'] = net(x, node_adaptation_s=True).numpy()
        out['node_t'] = net(x, node_adaptation_t=True).numpy()
        gf, fo = net(x, mid_feat=True)
        out['mid_x'], out['mid_feat'] = gf.numpy(), fo.numpy()
        out['cls_logits'] = cls(x).numpy()

    # gradients of a fixed scalar loss: fp32, then fp64 on the same fp32 metadata
    def grads(model, xin, meta_in):
        model.zero_grad()
        orig = model.g.preprocessor.forward
        model.g.preprocessor.forward = lambda pts: meta_in
        try:
            sem = model(xin, semantic_adaption=True)
            ns = model(xin, node_adaptation_s=True)
        finally:
            model.g.preprocessor.forward = orig
        loss_of((sem[0], sem[1], sem[2], sem[3], ns), None).backward()
        return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    g32 = grads(net, x, meta)
    meta64 = dict(meta)
    meta64['points'] = [p.double() for p in meta['points']]
    net64 = net.double()
    g64 = grads(net64, x.double(), meta64)
    names = sorted(g32)
    out['grad_names'] = np.array(names)
    out['grad_norm32'] = np.array([g32[k].double().norm().item() for k in names])
    out['grad_norm64'] = np.array([g64[k].norm().item() for k in names])
    out['grad_err32'] = np.array([(g32[k].double() - g64[k]).norm().item() for k in names])
    for k in SMALL_GRADS:
        out['grad32:' + k] = g32[k].numpy()
        out['grad64:' + k] = g64[k].numpy()
    path = os.path.join(HERE, 'kpconv.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
