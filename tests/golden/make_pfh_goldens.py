#!/usr/bin/env python3
"""Generate tests/golden/pfh.npz by RUNNING THE REFERENCE (build container only, CPU, about a minute).

Usage (from the repo root):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pfh_goldens.py

The reference's utils/pfh.py is imported as it is (matplotlib on the Agg backend; scipy is present) and its
PFH(e=0.1, div, nneighbors=8, rad).calc_normals / calcHistArray run on every case of tests/pfh_cases.CASES, its
pfh_hist_distance on every ordered pair of cases with equal div (a case against itself included).

The clouds are "shells" (pfh_cases.shell with the reference's own normal_pc and fps): random directions scaled by
U(0.7, 1) * (1, 0.7, 0.5), 4N points, normal_pc, fps to N, snapped to fp32 and handed to the reference as float64.  A
cloud is redrawn until every condition below holds; they are asserted on what is stored:
  - every point is used and has >= 3 neighbours (so the reference runs: no isolated point);
  - every normal's relative eigen gap (l_mid - l_min) / l_max is >= 1e-6, and |normal . p| >= 1e-9 (the re-orientation
    test of utils/pfh.py:297 cannot flip);
  - every feature is >= 1e-9 from every threshold, |a - b| >= 1e-9 and |a|, |b| <= 1 - 1e-9 (the arccos comparison);
  - consecutive candidate distances up to the (k+1)-th, and every distance and rad, are >= 1e-9 apart.
With these the bin counts and the neighbour lists are the same for every fp64 evaluation order, which is what lets the
tests ask for them exactly.

Per case the file holds pts fp32 [N, 3], counts uint8 [N, div^3] (the reference's histogram is counts / 36 bit for bit:
asserted), normals fp64 [N, 3], nbr int16 [N, 8], gap fp64 [N]; and dist_<S>__<T> fp64 for the distances.
"""
import itertools
import os
import sys

import numpy as np
import matplotlib
matplotlib.use('Agg')

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('SUG_REFERENCE', '/root/reference')
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)

import utils.pfh as r_pfh             # noqa: E402  (reference)
import pfh_cases as C                 # noqa: E402


def reference(pts, rad, div, k):
    """-> (hist [N, D], normals [N, 3], lists, used_idx) of the reference on the cloud in float64."""
    pc = np.asarray(pts, dtype=np.float64)
    d = r_pfh.PFH(e=0.1, div=div, nneighbors=k, rad=rad)
    norm, inds, used = d.calc_normals(pc)
    hist = d.calcHistArray(pc[used], norm, inds, used)
    return hist, np.array([np.asarray(n).reshape(3) for n in norm]), inds, used


def conditions(pts, rad, div, k, nrm, idx, cnt):
    """The margins of the stored cloud, from the REFERENCE's normals and lists -> (ok, text, gap, counts)."""
    P = np.asarray(pts, dtype=np.float64)
    _, _, m_n = C.neighbours(P, rad, k)
    _, gap, dots = C.normals(P, idx, cnt)
    counts, m_h, ab_max = C.hist_counts(P, nrm, idx, cnt, div)
    ok = (cnt.min() >= min(3, k) and gap.min() >= C.GAP and dots.min() >= C.MARGIN and m_n >= C.MARGIN and m_h >= C.MARGIN
          and ab_max <= 1 - C.MARGIN)
    text = 'neighbours %d..%d, gap %.1e, |n.p| %.1e, distance margin %.1e, feature margin %.1e, largest |a|, |b| %.3f' % (
        cnt.min(), cnt.max(), gap.min(), dots.min(), m_n, m_h, ab_max)
    return ok, text, gap, counts


def main():
    g = np.random.default_rng(20262)
    out, clouds = {}, {}
    for name, (N, rad, div, k) in C.CASES.items():
        for attempt in itertools.count():
            pts = clouds[C.SAME_CLOUD[name]] if name in C.SAME_CLOUD else C.shell(N, g, r_pfh.normal_pc, r_pfh.fps)
            try:
                hist, nrm, inds, used = reference(pts, rad, div, k)
            except IndexError:
                assert name not in C.SAME_CLOUD
                print('%s: draw %d has an isolated point (the reference raises), redrawn' % (name, attempt))
                continue
            if len(used) == N:
                cnt = np.array([len(l) for l in inds])
                idx = np.full((N, k), -1, dtype=np.int64)
                for i, l in enumerate(inds):
                    idx[i, :len(l)] = l
                ok, text, gap, counts = conditions(pts, rad, div, k, nrm, idx, cnt)
                if ok:
                    break
                print('%s: draw %d fails a condition (%s), redrawn' % (name, attempt, text))
            assert name not in C.SAME_CLOUD, name
        clouds[name] = pts
        # the restatement's lists and counts on the reference's normals are the reference's; its histogram is counts / 36
        r_idx, r_cnt, _ = C.neighbours(np.asarray(pts, dtype=np.float64), rad, k)
        assert np.array_equal(r_idx, idx) and np.array_equal(r_cnt, cnt), name
        assert np.array_equal(hist, counts / float(C.npairs(k))), name
        assert counts.max() <= 255 and (counts.sum(axis=1) == (cnt + 1) * cnt // 2).all()
        if name == 'n9_d2':
            assert (cnt == k).all()
        out[name + '_pts'] = pts
        out[name + '_counts'] = counts.astype(np.uint8)
        out[name + '_normals'] = nrm
        out[name + '_nbr'] = idx.astype(np.int16)
        out[name + '_gap'] = gap
        out[name + '_hist'] = hist                      # kept for the distances below, not stored
        print('%-8s N=%-3d rad=%.2f div=%d  %s' % (name, N, rad, div, text))
    hists = {name: out.pop(name + '_hist') for name in C.CASES}
    for s, t in itertools.product(C.CASES, C.CASES):
        if C.CASES[s][2] == C.CASES[t][2]:
            out['dist_%s__%s' % (s, t)] = np.float64(r_pfh.pfh_hist_distance(hists[s], hists[t]))
            print('distance %-8s -> %-8s %.17g' % (s, t, out['dist_%s__%s' % (s, t)]))
    path = os.path.join(HERE, 'pfh.npz')
    np.savez_compressed(path, **out)
    print('wrote %s  %.1f KB' % (path, os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 200 * 1000


if __name__ == '__main__':
    main()
