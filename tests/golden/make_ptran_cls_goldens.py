#!/usr/bin/env python3
"""Generate tests/golden/ptran_cls.npz by RUNNING THE REFERENCE's PointTransformerCls (build container only, CPU).

Usage (from the repo root, ~2 min):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ptran_cls_goldens.py

Uses make_goldens.py's set-up (stub modules, the 'cuda' -> 'cpu' redirect, the parameter fill and probes).  The
reference's Ptran_model.py builds its default cfg with easydict, which is not installed: an attribute dict that turns
nested dicts into attribute dicts on assignment (what EasyDict does) stands in for it.

Recorded per cloud size (B = 2, N = 1024 and 2048; prefix n<N>_), the model from a seed (oracle.ref_cpu.fill_params), not
its weights:
  * train mode, the FPS starts drawn from the CPU generator after torch.manual_seed(seed + 1): logits, CE loss, per
    parameter the gradient norm and the dot with a seeded probe, in fp32 and (same draws) in fp64; BatchNorm buffers;
  * one torch.optim.Adam step in train_source.py's form (lr 5e-4, weight decay 1e-4): per parameter the sum and the
    norm of the change, then the CE loss of a second forward (torch.manual_seed(seed + 2));
  * eval-mode logits after the step (torch.manual_seed(seed + 3)).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG                 # noqa: E402  (stubs, cuda -> cpu redirect, reference on sys.path)


class _AttrDict(dict):
    """easydict.EasyDict stand-in: attribute access, nested dicts become attribute dicts on assignment."""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setitem__(self, k, v):
        super().__setitem__(k, _AttrDict(v) if isinstance(v, dict) and not isinstance(v, _AttrDict) else v)

    __setattr__ = __setitem__


sys.modules['easydict'].EasyDict = _AttrDict
import model.Ptran_model as r_PT           # noqa: E402  (reference)

from oracle import ref_cpu as O            # noqa: E402

B = 2
LR, WD = 5e-4, 1e-4                        # train_source.py:94 with the PTran values of the shipped yaml


def _grads(net, x, lab, seed):
    torch.manual_seed(seed + 1)
    y = net(x)
    loss = torch.nn.functional.cross_entropy(y, lab)
    net.zero_grad()
    loss.backward()
    names, norm, dot = [], [], []
    for k, v in net.named_parameters():
        if v.grad is None:
            continue
        names.append(k)
        norm.append(v.grad.double().norm().item())
        dot.append((v.grad.double() * MG._probe(v.shape, 'g' + k).double()).sum().item())
    return y, loss, names, np.array(norm), np.array(dot)


def gen(N, seed, out):
    pre = 'n%d_' % N
    g = torch.Generator().manual_seed(seed)
    x = O.synth_clouds(B, N, g)
    lab = torch.randint(0, 10, (B,), generator=g)
    net = r_PT.PointTransformerCls()
    p0 = MG._load(net, seed)
    net.train()
    sd = net.state_dict()
    if 'keys' not in out:
        out['keys'] = np.array(list(sd.keys()))
        out['shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    y, loss, names, gn, gd = _grads(net, x, lab, seed)
    sd1 = net.state_dict()
    bn_names = [k for k in sd1 if k.endswith('running_mean') or k.endswith('running_var')]
    # fp64: same parameters, same FPS draws
    net64 = r_PT.PointTransformerCls()
    net64.load_state_dict(p0)
    net64 = net64.double().train()
    y64, loss64, names64, gn64, gd64 = _grads(net64, x.double(), lab, seed)
    assert names64 == names
    MG.same(y, y64.float(), 'fp32 vs fp64 logits', 1e-4)
    out.update({pre + 'x': x, pre + 'label': lab, pre + 'seed': seed, pre + 'y': y, pre + 'loss': loss,
                pre + 'y64': y64, pre + 'loss64': loss64.item(),
                pre + 'grad_names': np.array(names), pre + 'grad_norm': gn, pre + 'grad_dot': gd,
                pre + 'grad_norm64': gn64, pre + 'grad_dot64': gd64,
                pre + 'bn_names': np.array(bn_names),
                pre + 'bn_sum': np.array([sd1[k].double().sum().item() for k in bn_names])})
    # one Adam step (train_source.py:94, :113-131), then a second forward
    opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=WD)
    opt.step()
    opt.zero_grad()
    post = dict(net.named_parameters())
    pnames = [k for k, _ in net.named_parameters()]
    out[pre + 'param_names'] = np.array(pnames)
    out[pre + 'param_sum'] = np.array([post[k].detach().double().sum().item() for k in pnames])
    out[pre + 'param_delta_norm'] = np.array([(post[k].detach() - p0[k]).double().norm().item() for k in pnames])
    torch.manual_seed(seed + 2)
    with torch.no_grad():
        out[pre + 'loss2'] = torch.nn.functional.cross_entropy(net(x), lab).item()
    net.eval()
    torch.manual_seed(seed + 3)
    with torch.no_grad():
        out[pre + 'y_eval'] = net(x)
    print('N=%d: loss %.6f (fp64 %.6f), after one Adam step %.6f' % (N, loss.item(), loss64.item(), out[pre + 'loss2']))


if __name__ == '__main__':
    torch.set_num_threads(8)
    out = {}
    gen(1024, 61, out)
    gen(2048, 62, out)
    MG.save('ptran_cls.npz', **out)
