"""CPU: graph_replay.ReplayedStep's plan / capture / replay protocol driven with fakes (a graph that counts its replays, a
capture that runs its body, a feeder that counts build / refill), and the small helpers the step classes share."""
import contextlib

import pytest
import torch
import torch.nn as nn

from sug_amd import graph_replay
from sug_amd.graph_replay import ReplayedStep, adam_choice, plain_ce, refusal_text

B = 4


class FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


class FakeFeeder:
    made = []

    def __init__(self, device):
        self.builds = self.refills = 0
        FakeFeeder.made.append(self)

    def recording(self):
        return contextlib.nullcontext()

    def providing(self):
        return contextlib.nullcontext()

    def build(self):
        self.builds += 1

    def refill(self):
        self.refills += 1


@pytest.fixture
def captures(monkeypatch):
    """The graphs handed to the fake torch.cuda.graph, in order: one per capture entered."""
    entered = []

    def fake_graph(g, *a, **k):
        entered.append(g)
        return contextlib.nullcontext()

    FakeFeeder.made = []
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', FakeGraph)
    monkeypatch.setattr(torch.cuda, 'graph', fake_graph)
    monkeypatch.setattr(graph_replay, 'StartFeeder', FakeFeeder)
    return entered


class Step(ReplayedStep):
    def __init__(self, captures, tuple_out=False):
        super().__init__(max_graphs=4, rows=2)
        self.use_graph = True
        self.params = [nn.Parameter(torch.ones(2)), nn.Parameter(torch.ones(2))]
        self.opts = tuple(torch.optim.SGD([p], lr=0.1) for p in self.params)
        for o in self.opts:
            o.plan_generation = 0
        self.captures, self.seen = captures, len(captures)
        self.tuple_out = tuple_out
        self.calls = self.calls_in_capture = 0
        self.fail_in_capture = False
        self.grads_none_on_entry = []

    def _opts(self):
        return self.opts

    def _graph_key(self, batch):
        return tuple(tuple(t.shape) for t in batch)

    def _eager_step(self, x, y):
        in_capture = len(self.captures) != self.seen        # torch.cuda.graph was entered since the last call
        self.seen = len(self.captures)
        self.calls += 1
        self.calls_in_capture += in_capture
        self.grads_none_on_entry.append(all(p.grad is None for p in self.params))
        if in_capture and self.fail_in_capture:
            for p in self.params:                           # what an aborted capture leaves behind
                p.grad = torch.ones_like(p)
            raise RuntimeError('not capturable\nsecond line')
        self._rows_host[0] += x.shape[0]
        loss = x.sum() + y.sum()
        return (loss, loss + 1) if self.tuple_out else loss


def batch(b=B):
    return torch.ones(b, 3), torch.ones(b)


def test_plan_capture_replay_counts_and_host_rows(captures):
    tr = Step(captures)
    outs = [tr._graph_step(batch()) for _ in range(2)]
    assert tr.stats == {'planned': 1, 'captured': 1, 'replayed': 1, 'refused': 0}
    outs.append(tr._graph_step(batch()))
    assert tr.stats == {'planned': 1, 'captured': 1, 'replayed': 2, 'refused': 0}
    (fd,), (st,) = FakeFeeder.made, tr._graphs.values()
    assert fd.builds == 1 and fd.refills == 2 and st['graph'].replays == 2 and captures == [st['graph']]
    assert tr.calls == 2 and tr.calls_in_capture == 1      # the plan and the capture; a replay runs no Python step
    assert tr._rows_host == [3 * B, 0]                      # the capture's own count taken back, one delta per replay
    assert st['rows'] == (B, 0)
    for o in outs:
        assert isinstance(o, torch.Tensor) and float(o) == 4 * B
        assert o.data_ptr() != st['out'].data_ptr()
    assert outs[1].data_ptr() != outs[2].data_ptr()


def test_tuple_output_comes_back_as_a_tuple_of_one_clone(captures):
    tr = Step(captures, tuple_out=True)
    outs = [tr._graph_step(batch()) for _ in range(3)]
    (st,) = tr._graphs.values()
    assert st['out'].shape == (2,)                          # stacked inside the capture
    for o in outs:
        assert isinstance(o, tuple) and len(o) == 2 and [float(v) for v in o] == [4 * B, 4 * B + 1]
    a, b = outs[2]
    assert a.data_ptr() != st['out'].data_ptr() and b.data_ptr() == a.data_ptr() + a.element_size()


def test_an_input_that_is_the_static_tensor_is_not_copied(captures):
    tr = Step(captures)
    for _ in range(2):
        tr._graph_step(batch())
    (st,) = tr._graphs.values()
    x_static, y_static = st['in']
    vx, vy = x_static._version, y_static._version
    tr._graph_step((x_static, torch.full((B,), 2.0)))
    assert x_static._version == vx and y_static._version == vy + 1
    assert y_static.tolist() == [2.0] * B


def test_a_failed_capture_keeps_the_key_eager_for_good(captures):
    tr = Step(captures)
    tr.fail_in_capture = True
    tr._graph_step(batch())
    out = tr._graph_step(batch())
    assert tr.stats == {'planned': 1, 'captured': 0, 'replayed': 0, 'refused': 1}
    assert tr.why == refusal_text(RuntimeError('not capturable\nsecond line')) == 'RuntimeError: not capturable'
    assert float(out) == 4 * B                              # the eager result
    assert tr.grads_none_on_entry == [True, True, True]     # plan, capture, and the eager step after zero_grad(set_to_none)
    assert all(p.grad is None for p in tr.params)
    (st,) = tr._graphs.values()
    assert st['why'] == tr.why and st['graph'] is None and st['in'] is None and st['out'] is None
    for _ in range(2):
        assert float(tr._graph_step(batch())) == 4 * B
    assert len(captures) == 1 and tr.calls_in_capture == 1 and tr.calls == 5
    assert tr._rows_host == [4 * B, 0]
    tr.fail_in_capture = False
    for _ in range(3):                                      # another key still captures
        tr._graph_step(batch(3))
    assert tr.stats == {'planned': 2, 'captured': 1, 'replayed': 2, 'refused': 1} and len(captures) == 2


def test_a_new_plan_generation_releases_the_entry_and_plans_again(captures):
    tr = Step(captures)
    for _ in range(2):
        tr._graph_step(batch())
    (old,) = tr._graphs.values()
    assert old['gens'] == (0, 0) and old['graph'] is not None
    tr.opts[1].plan_generation = 1
    tr._graph_step(batch())
    assert old['graph'] is None and old['in'] is None and old['out'] is None
    (new,) = tr._graphs.values()
    assert new is not old and tr.stats['planned'] == 2 and tr.stats['replayed'] == 1
    tr._graph_step(batch())
    assert new['gens'] == (0, 1) and tr.stats['captured'] == 2


def test_max_graphs_set_after_construction_bounds_the_entries(captures):
    tr = Step(captures)
    for _ in range(2):
        tr._graph_step(batch())
    (first,) = tr._graphs.values()
    assert first['graph'] is not None
    tr.max_graphs = 1
    seen = [first]
    for i in range(6):
        tr._graph_step(batch(3 if i % 2 == 0 else B))
        assert len(tr._graphs) == 1
        seen += [st for st in tr._graphs.values() if all(st is not s for s in seen)]
        for st in seen:
            if all(st is not kept for kept in tr._graphs.values()):
                assert st['graph'] is None and st['in'] is None and st['out'] is None
    assert len(seen) == 7 and tr.stats['planned'] == 7


# ----------------------------------------------------------------------------- the small helpers
def test_pack_and_unpack_columns_round_trip():
    from sug_amd.train_step import pack_columns, unpack_columns
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn(5, 7, generator=g), torch.randint(-3, 40, (5,), generator=g), torch.randn(5, 2, 3, generator=g)]
    packed, meta = pack_columns(ts)
    assert packed.shape == (5, 7 + 1 + 6) and packed.dtype == torch.float32
    back = unpack_columns(packed, meta)
    assert len(back) == len(ts)
    for a, b in zip(ts, back):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def test_grads_as_views_point_into_the_flat_buffer():
    from sug_amd.train_step import _grads_as_views
    ps = [nn.Parameter(torch.zeros(2, 3)), nn.Parameter(torch.zeros(5)), nn.Parameter(torch.zeros(1, 2, 2))]
    flat = torch.arange(15, dtype=torch.float32)
    _grads_as_views(ps, flat)
    off = 0
    for p in ps:
        assert p.grad.shape == p.shape
        assert p.grad.data_ptr() == flat.data_ptr() + off * flat.element_size()
        assert torch.equal(p.grad.reshape(-1), flat[off:off + p.numel()])
        off += p.numel()
    assert off == flat.numel()


def test_adam_choice_on_cpu_is_torch_adam_without_extras():
    assert adam_choice(False, None, False) == (torch.optim.Adam, {})
    assert adam_choice(False, True, False) == (torch.optim.Adam, {})
    assert adam_choice(True, False, False) == (torch.optim.Adam, {})
    assert adam_choice(True, False, True) == (torch.optim.Adam, {'capturable': True, 'fused': True})
    from sug_amd.optim import Adam
    for use_graph in (False, True):
        assert adam_choice(True, None, use_graph) == (Adam, {'graph_capturable': True})


def test_plain_ce_with_and_without_smoothing():
    assert plain_ce(nn.CrossEntropyLoss()) and plain_ce(nn.CrossEntropyLoss(ignore_index=3), smoothing_ok=True)
    smooth = nn.CrossEntropyLoss(label_smoothing=0.1)
    assert not plain_ce(smooth) and plain_ce(smooth, smoothing_ok=True)
    for c in (nn.CrossEntropyLoss(weight=torch.ones(4)), nn.CrossEntropyLoss(reduction='sum'), nn.NLLLoss(),
              type('Mine', (nn.CrossEntropyLoss,), {})()):
        assert not plain_ce(c) and not plain_ce(c, smoothing_ok=True)
