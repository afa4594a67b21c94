"""utils/pfh.py on the device: Point Feature Histograms of resident clouds and the histogram cloud distance.

The reference loops over points and pairs in Python, one process per cloud; here all clouds of a call go through ONE launch of
sug_pfh_descriptors (one workgroup per cloud) and one source against M targets through one launch of sug_pfh_hist_distance.
The semantics -- neighbours, normals, pair features, bins, and what happens to a point without a neighbour -- are written
next to the two declarations in include/sug_amd.h.  Everything refuses CPU tensors and writes no files.

    pcs = process_pts(raw, pt_num=500)                      # [M, 500, 3]
    hists, ok = get_pfh_descriptor(pcs)                     # [M, 500, 8] fp64, ok[m]: every point of cloud m has a neighbour
    d = pfh_hist_distance(hists[anchor], hists)             # [M] fp64

Not mirrored, because the reference's own versions cannot run and so nothing can pin them: SPFH and FPFH (their calcHistArray
takes three arguments where PFH.findMatches and get_pfh_descriptor_worker pass three and four of another meaning, and index
norm[j] by list position) and PFH.solve (findMatches unpacks calc_normals' three results into two names).
"""
import numpy as np
import torch

from .. import ops
from ..dataset_splitter import process_pts            # noqa: F401  (re-exported, as the reference defines it here too)

# get_pfh_descriptor's PFH(e=0.1, div=2, nneighbors=8, rad=0.2) (utils/pfh.py:117)
DEFAULT_E, DEFAULT_DIV, DEFAULT_NNEIGHBORS, DEFAULT_RAD = 0.1, 2, 8, 0.2


def _batched(pc, what):
    ops._need_gpu(pc)
    if pc.dim() not in (2, 3) or pc.shape[-1] < 3:
        raise ValueError('%s: expected a cloud [N, C>=3] or clouds [M, N, C>=3], got %s' % (what, tuple(pc.shape)))
    x = pc[..., :3].to(torch.float32)
    return (x.unsqueeze(0) if pc.dim() == 2 else x).contiguous(), pc.dim() == 2


class PFH(object):
    """PFH(e, div, nneighbors, rad) of utils/pfh.py:162-177.  `e` is the stopping threshold of solve(), which is not
    mirrored; it is kept so that the constructor takes the reference's arguments."""

    def __init__(self, e, div, nneighbors, rad):
        if not 2 <= int(div) <= 5:
            raise ValueError('PFH: div=%r outside 2 .. 5' % (div,))
        if not 1 <= int(nneighbors) <= ops.PFH_MAX_NEIGHBORS:
            raise ValueError('PFH: nneighbors=%r outside 1 .. %d' % (nneighbors, ops.PFH_MAX_NEIGHBORS))
        self._e = e
        self._div = int(div)
        self._nneighbors = int(nneighbors)
        self._radius = float(rad)
        self._last = None

    def describe(self, pc):
        """One launch for a cloud [N, 3] or clouds [M, N, 3]: (hist, normals, nbr_idx, nbr_cnt, used_cnt) as
        ops.pfh_descriptors returns them, without the batch axis for a single cloud."""
        x, single = _batched(pc, 'PFH')
        out = ops.pfh_descriptors(x, self._radius, self._nneighbors, self._div)
        out = tuple(o[0] for o in out) if single else out
        self._last = (pc, pc._version, out)
        return out

    def _described(self, pc):
        if self._last is not None and self._last[0] is pc and self._last[1] == pc._version:
            return self._last[2]
        return self.describe(pc)

    def calc_normals(self, pc):
        """calc_normals of utils/pfh.py:270-301 -> (normals fp64 [..., N, 3], neighbour lists int32 [..., N, k] padded with
        -1, used mask bool [..., N]).  The reference returns lists over the used points only; here every point keeps its row
        (an unused one: a zero normal, a list of -1) and the mask says which rows count."""
        _, normals, nbr_idx, nbr_cnt, _ = self.describe(pc)
        return normals, nbr_idx, nbr_cnt > 0

    def calcHistArray(self, pc, norm=None, indNeigh=None, used_idx=None):
        """calcHistArray of utils/pfh.py:303-348 -> fp64 [..., N, div^3], an unused point's row zero.  The kernel forms
        neighbours, normals and histograms in one launch, so the histograms are always those of pc's own normals: norm,
        indNeigh and used_idx are accepted for the reference's call shape and must be None or what calc_normals(pc)
        returned (then that launch's result is used, not a second launch)."""
        last = self._last
        for given, slot in ((norm, 1), (indNeigh, 2)):
            if given is not None and (last is None or last[0] is not pc or given is not last[2][slot]):
                raise ValueError('PFH.calcHistArray: norm / indNeigh must be what calc_normals(pc) returned for this cloud; '
                                 'the histograms of other normals are not computed')
        return self._described(pc)[0]

    def calc_thresholds(self):
        """calc_thresholds of utils/pfh.py:481-495: a 3 x (div - 1) host array, the thresholds of alpha, phi, theta (the
        launcher forms the same values with the same operations)."""
        delta = 2. / self._div
        s1 = np.array([-1 + i * delta for i in range(1, self._div)])
        s3 = np.array([-1 + i * delta for i in range(1, self._div)])
        delta = np.pi / self._div
        s4 = np.array([-np.pi / 2 + i * delta for i in range(1, self._div)])
        return np.array([s1, s3, s4])

    def solve(self, P, Q):
        raise NotImplementedError('PFH.solve is not mirrored: in the reference findMatches unpacks the three results of '
                                  'calc_normals into two names and calls calcHistArray with three arguments, so it cannot run '
                                  'and nothing pins it')


class SPFH(PFH):
    def calcHistArray(self, pc, norm=None, indNeigh=None, used_idx=None):
        raise NotImplementedError('SPFH is not mirrored: the reference\'s SPFH.calcHistArray takes (pc, norm, indNeigh) while its '
                                  'only caller passes four arguments, and indexes norm[j] by list position; it cannot run and '
                                  'nothing pins it')


class FPFH(PFH):
    def calcHistArray(self, pc, norm=None, indNeigh=None, used_idx=None):
        raise NotImplementedError('FPFH is not mirrored: the reference\'s FPFH.calcHistArray takes (pc, norm, indNeigh) while its '
                                  'only caller passes four arguments, and indexes norm[j] by list position; it cannot run and '
                                  'nothing pins it')


def get_pfh_descriptor(pcs, dataset_type=None, method='PFH'):
    """get_pfh_descriptor of utils/pfh.py:116-143 with its PFH(0.1, 2, 8, 0.2): pcs [M, N, 3] -> (hists fp64 [M, N, 8],
    status bool [M]), all clouds in one launch.  status[m] is True where every point of cloud m has a neighbour -- the
    clouds the reference itself can process; elsewhere its worker raises and the cloud is "skipped", here the isolated
    points have zero rows and take no part in distances.  dataset_type only named the reference's output files: nothing is
    written."""
    if method != 'PFH':
        raise NotImplementedError('get_pfh_descriptor: method=%r: only PFH can run in the reference (see SPFH, FPFH)' % (method,))
    ops._need_gpu(pcs)
    if pcs.dim() != 3:
        raise ValueError('get_pfh_descriptor: expected clouds [M, N, C>=3], got %s' % (tuple(pcs.shape),))
    hist, _, _, _, used_cnt = PFH(DEFAULT_E, DEFAULT_DIV, DEFAULT_NNEIGHBORS, DEFAULT_RAD).describe(pcs)
    return hist, used_cnt == pcs.shape[1]


def _used_rows(hist):
    # a used point has at least one neighbour, so at least one pair, so a row that is not all zero; an unused one a zero row
    return (hist != 0).any(dim=-1).to(torch.int32)


def pfh_hist_distance(histS, histT):
    """pfh_hist_distance of utils/pfh.py:146-159: histS [Ns, D]; histT [Nt, D] -> a 0-dim fp64 device tensor, or
    [M, Nt, D] -> [M] in one launch.  Zero rows (points without a neighbour) are left out on both sides."""
    ops._need_gpu(histS, histT)
    single = histT.dim() == 2
    tgt = (histT.unsqueeze(0) if single else histT).to(torch.float64)
    src = histS.to(torch.float64)
    d = ops.pfh_hist_distance(src, _used_rows(src), tgt, _used_rows(tgt))
    return d[0] if single else d
