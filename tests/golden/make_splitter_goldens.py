#!/usr/bin/env python3
"""Generate tests/golden/splitter.npz from the numpy fp64 restatement in tests/splitter_cases.py (CPU, a few seconds):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_splitter_goldens.py

The fixture holds the synthetic inputs (96 clouds of 64 points, 8 pairs of 61 x 77 points, 2 pairs of 500 x 500 points,
one thin cylinder,
257 rows of probabilities, 4 raw clouds of 128 points) and what the restatement computes from them: count, rmse, iters
and transform at max_iteration 0, 1 and 30, the split labels for fixed anchors, the entropy clusters, the sampled points.

The tests compare a kernel with this restatement at rounding level, which is meaningful only away from the restatement's
own discontinuities.  So the generator ASSERTS, and a change of seeds that breaks one of these fails here, not in a test:
  * no nearest-neighbour d2 of any evaluation lies within 1e-9 relative of r*r (a count cannot flip on the last bit);
  * every first update's Sigma has its two smallest singular values at least 1e-3 apart and at least 1e-3 from zero (the
    rotation is well conditioned: first-order perturbation theory bounds its error by the data error over that gap);
  * every farthest-point step of the process_pts case wins by a relative margin of at least 1e-4, and no entropy lies
    within 1e-5 of a histogram edge it does not define (fp32 inputs move these by 1e-7 at most);
  * the mean cut accepts the class's first anchor, the histogram cut refuses all five (the fifth try is kept), and the
    redraw class fails the balance test on its first anchor and passes on its second."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import splitter_cases as C                # noqa: E402


def check_preconditions(fx, out, traces):
    for name, trs in traces.items():
        for b, tr in enumerate(trs):
            assert tr['r2_margin'] > 1e-9, (name, b, tr['r2_margin'])
            if 'sv' in tr:
                s = tr['sv']
                assert s[1] - s[2] >= 1e-3 and s[2] >= 1e-3, (name, b, s)
                assert out['%s_it1_count' % name][b] >= 3, (name, b)
    assert out['process_margin'] >= 1e-4, out['process_margin']
    for k in (2, 4):
        assert C.edge_margin(out['ent_u'], k) >= 1e-5, (k, C.edge_margin(out['ent_u'], k))
    assert out['split_mean_tries'] == 1 and out['split_hist_tries'] == 5
    assert out['redraw_tries'] == 2


if __name__ == '__main__':
    fx = C.inputs()
    traces = {}
    out = C.results(fx, traces)
    check_preconditions(fx, out, traces)
    for name in C.PAIR_SETS:
        print('%-4s it30: iters %s, count %s' % (name, np.bincount(out[name + '_it30_iters']).tolist(),
                                                 out[name + '_it30_count'].tolist()))
    print('labels mean: %d zeros, hist: %d zeros, redraw: %d zeros' % tuple(
        int((out[k] == 0).sum()) for k in ('split_mean_labels', 'split_hist_labels', 'redraw_labels')))
    path = os.path.join(HERE, 'splitter.npz')
    np.savez_compressed(path, **fx, **out)
    size = os.path.getsize(path)
    print('%s: %d bytes' % (path, size))
    assert size < 200 * 1000, 'the fixture has %d bytes' % size
