"""sug_eval_accumulate and the drop-in eval_worker on the GPU (the cases: tests/eval_worker_cases.py).

The cases run in ONE child process started by the module fixture: the runners of sug_amd.eval_graphs keep private model copies
and graph pools alive by design, and this test process must hand the tests after this file the caching-allocator history it
would have without them.  Each test reports its case."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KINDS = ('DGCNN', 'Pointnet', 'Pointnet2', 'PTran', 'Pointnet_cls')


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('eval_worker') / 'results.json')
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(ROOT, 'tests', 'eval_worker_cases.py'), out]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    res = json.load(open(out)) if os.path.exists(out) else {}
    return res, r


def _check(cases, name):
    res, r = cases
    if name not in res:
        pytest.fail('the case process ended (exit %d) before case %s:\n%s' % (r.returncode, name, r.stderr.decode()[-3000:]))
    assert res[name] is None, res[name]


def test_kernel_against_torch_and_graph_capture(cases):
    """Predictions equal torch.max on the device (ties, a row of equal values, a NaN row); counts, class_acc and batch_acc
    equal the restated torch / numpy loop bit for bit, the loss within 1e-6; a captured replay equals eager launches; a
    label outside [0, C) sets the error word."""
    _check(cases, 'kernel_against_torch_and_graph_capture')


@pytest.mark.parametrize('kind', KINDS)
def test_eval_worker_two_epochs_equal_the_eager_loop(cases, kind):
    """Two epochs on fresh deep copies, the second after perturbing every parameter: result dict, class_acc, instance_acc
    exact, loss within 1e-6, CPU generator state equal, every batch of epoch 2 replayed (the partial one included)."""
    _check(cases, 'eval_worker_two_epochs_equal_the_eager_loop[%s]' % kind)


def test_fallbacks_give_identical_results(cases):
    """Train mode, focal_loss (called once per batch, alpha as after the eager loop), cls_eval=False."""
    _check(cases, 'fallbacks_give_identical_results')


def test_replays_see_weights_after_training_steps(cases):
    """DGCNN after SUGStep(share_prefix=True) steps (cache_weight_split on): evaluations before and after one more step equal
    the eager evaluation of the same weights."""
    _check(cases, 'replays_see_weights_after_training_steps')
