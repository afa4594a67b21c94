"""ChamferDistance: the op the reference's model/mmd.py imports from the third-party `chamfer_distance` package
(`from chamfer_distance import ChamferDistance`), here on the library's own HIP kernels (sug_chamfer_nn / sug_chamfer_nn_bwd).

    from sug_amd.chamfer_distance import ChamferDistance
    dist1, dist2, idx1, idx2 = ChamferDistance()(xyz1, xyz2)

The third-party op is a CUDA extension built at import time and is absent wherever this package runs, so its behaviour is
restated from its call sites (cd_distance, model/mmd.py:169-175) and parity is unpinned, as it is for sug_chamfer.  In
particular the dtype of its index outputs cannot be checked here: the indices leave as int64, like every index this package
hands to Python.  On exact ties the lowest index is returned.  Out of scope: second-order gradients, the call form
`ChamferDistance(pc_1, pc_2)` of the reference's KPC=True branch (model/mmd.py:123: the class called with two clouds), and
point dimensions other than 3."""
import torch.nn as nn

from . import ops


def chamfer_distance(xyz1, xyz2):
    """xyz1 [B,N,3], xyz2 [B,M,3] fp32 rows on the HIP device -> (dist1 [B,N], dist2 [B,M], idx1 [B,N], idx2 [B,M]):
    dist1[b,i] = min_j |xyz1[b,i] - xyz2[b,j]|^2 and idx1[b,i] the lowest j attaining it (int64, no gradient); dist2 / idx2
    the same for xyz2 against xyz1.  Both distances are differentiable with respect to both clouds (first order)."""
    dist1, dist2, idx1, idx2 = ops.chamfer_nn(xyz1, xyz2)
    return dist1, dist2, idx1.long(), idx2.long()


class ChamferDistance(nn.Module):
    """Module form of chamfer_distance (no parameters, no state)."""

    def forward(self, xyz1, xyz2):
        return chamfer_distance(xyz1, xyz2)
