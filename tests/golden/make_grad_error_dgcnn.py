"""tests/golden/grad_error_dgcnn.npz: the fp32 oracle's gradient error against the fp64 oracle for the DGCNN case of
test_gpu_model.py::test_gradient_error_is_fp32_rounding_of_the_reference_arithmetic (weight seed 5, data seed 3, B = 4), on
the HIP path's four neighbour graphs, measured on the CPU the other goldens were made on.  Which of two near-tied maxima the
fp32 arithmetic picks depends on the CPU's sgemm summation order, so that figure is stored, not recomputed on each host.
usage: python tests/golden/make_grad_error_dgcnn.py GRAPHS.npz   (knn0..knn3: the HIP graphs, int16 [B, N, 20])"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from oracle import ref_cpu as O                      # noqa: E402
from test_gpu_model import probe                     # noqa: E402
from sug_amd.model.Model import Net_MDA              # noqa: E402

SEED, DATA_SEED, B = 5, 3, 4


def fp_gradients(rec):
    x = O.synth_clouds(B, 1024, torch.Generator().manual_seed(DATA_SEED))
    w1, w2 = probe((B, 10), 'w1'), probe((B, 256), 'w2')
    fill = O.fill_params({k: tuple(v.shape) for k, v in Net_MDA('DGCNN').state_dict().items()}, SEED)
    out = {}
    for dt in (torch.float32, torch.float64):
        p = O.as_params({k: (v.to(dt) if v.dtype.is_floating_point else v) for k, v in fill.items()})
        torch.manual_seed(SEED + 1)
        y1, y2, s1, s2 = O.net_mda(p, 'DGCNN', x.to(dt), True, None, semantic_adaption=True, knn_override=rec)
        ((y1 * w1.to(dt)).sum() + (y2 * w1.to(dt)).sum() + (s1 * w2.to(dt)).sum() + (s2 * w2.to(dt)).sum()).backward()
        out[dt] = {k: v.grad.double() for k, v in p.items() if v.requires_grad and v.grad is not None}
    return out[torch.float32], out[torch.float64]


if __name__ == '__main__':
    z = np.load(sys.argv[1])
    graphs = {'knn%d' % i: z['knn%d' % i].astype(np.int16) for i in range(4)}
    g32, g64 = fp_gradients([torch.from_numpy(graphs['knn%d' % i].astype(np.int64)) for i in range(4)])
    keys = sorted(g64)
    tot = sum(float(g64[k].norm()) ** 2 for k in keys) ** 0.5
    e_ref = sum(float((g32[k] - g64[k]).norm()) ** 2 for k in keys) ** 0.5 / tot
    own = [float((g32[k] - g64[k]).norm()) / max(float(g64[k].norm()), 1e-30) for k in keys]
    np.savez_compressed(os.path.join(HERE, 'grad_error_dgcnn.npz'), keys=np.array(keys), own_err=np.array(own),
                        e_ref=np.float64(e_ref), **graphs)
    print('fp32 oracle vs fp64: relative L2 %.3e over %d tensors (%d torch threads)' % (e_ref, len(keys), torch.get_num_threads()))
