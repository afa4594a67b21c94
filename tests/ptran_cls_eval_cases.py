"""The eval cases of tests/test_gpu_ptran_cls.py for PointTransformerCls: the graph-replayed eval forward against the eager
call, and eval_worker with source_flag against the restated reference loop of tests/eval_worker_cases.py.

Run as a script in a child process of its own (`python tests/ptran_cls_eval_cases.py RESULTS.json`), as
tests/eval_worker_cases.py is, so that the runners' private copies and graph pools do not change the caching-allocator
history of later tests.  Writes {case id: null | traceback}."""
import copy
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import ref_cpu as O  # noqa: E402
import eval_worker_cases as EC  # noqa: E402

B, N = 4, 1024


def _setup(seed=5):
    from sug_amd.model.Ptran_model import PointTransformerCls
    g = torch.Generator().manual_seed(seed)
    net = PointTransformerCls()
    net.load_state_dict(O.fill_params({k: tuple(v.shape) for k, v in net.state_dict().items()}, 3))
    net = net.cuda().train()
    torch.manual_seed(seed)
    with torch.no_grad():
        net(O.synth_clouds(B, N, g).cuda())                                     # BatchNorm running buffers
    net.eval()
    batches = []
    for b in (B, B, B, B // 2):                                                  # three full batches and a partial one
        batches.append((O.synth_clouds(b, N, g).cuda(), torch.randint(0, 9, (b,), generator=g).cuda()))   # class 9 unseen
    return net, batches


def case_graph_replay_equals_eager_call():
    from sug_amd import eval_graphs
    net, batches = _setup(7)
    runner = eval_graphs.EvalRunner(net)
    x = batches[0][0]
    for call in range(4):                       # eager, capture, replay, replay
        torch.manual_seed(20 + call)
        with torch.no_grad():
            want = copy.deepcopy(net)(x)
        torch.manual_seed(20 + call)
        got = runner(x)
        assert torch.equal(got, want), (call, float((got - want).abs().max()))
    assert runner.stats['captured'] == 1 and runner.stats['replayed'] >= 2 and runner.stats['refused'] == 0, runner.stats


def case_eval_worker_source_flag_two_epochs():
    from sug_amd import eval_graphs
    from sug_amd.utils.eval_utils import LAST
    net, batches = _setup()
    ce = nn.CrossEntropyLoss().cuda()
    res, ref = EC._epoch(net, batches, ce, 11, source_flag=True)
    EC._compare(res, ref)
    assert LAST['form'] == 'device' and LAST['graphs'] and LAST['syncs'] == 1
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.01 * torch.randn_like(p))                                   # the next epoch's weights
    runner = eval_graphs.runner_for(net)
    before = dict(runner.stats)
    res, ref = EC._epoch(net, batches, ce, 12, source_flag=True)
    EC._compare(res, ref)
    assert runner.stats['replayed'] - before['replayed'] == 4, runner.stats
    assert runner.stats['eager'] == before['eager'] and runner.stats['refused'] == 0, (runner.stats, runner.why)


CASES = [('graph_replay_equals_eager_call', case_graph_replay_equals_eager_call),
         ('eval_worker_source_flag_two_epochs', case_eval_worker_source_flag_two_epochs)]


def main(out_path):
    from sug_amd.model.Model import Net_MDA
    Net_MDA.call_graphs = False             # the form tests/conftest.py pins for every test
    res = {}
    for name, fn in CASES:
        try:
            fn()
            res[name] = None
        except Exception:
            res[name] = traceback.format_exc()
        with open(out_path, 'w') as fh:     # after every case: a crash leaves the results so far
            json.dump(res, fh)


if __name__ == '__main__':
    main(sys.argv[1])
