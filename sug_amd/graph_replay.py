"""What the three hipGraph front ends share (SUGStep's graph step, call_graphs.CallGraphs, eval_graphs.EvalRunner).

Each of them runs a key eagerly once under `StartFeeder.recording()`, captures it under `StartFeeder.providing()` and from
then on copies the inputs, calls `refill()` and replays.  The capture itself stays written out at each site, as
`with feeder.providing(), ops.capture_guard(), torch.cuda.graph(...)`; no context manager is entered on a replay path.
"""
import collections
import contextlib

import torch

from . import ops


class StartFeeder:
    """FPS start indices for a replayable forward / step: drawn from the CPU default generator in call
    order with the same (B, N) sequence as an eager run (so the random stream is the
    reference's, model/point_utils.py:17), but delivered through one static device buffer."""

    def __init__(self, device):
        self.device = device
        self.plan = []          # (B, N) per farthest_point_sample call
        self.host = self.dev = None
        self.cursor = 0

    def record(self, B, N):     # provider during the eager planning run
        self.plan.append((B, N))
        return torch.randint(0, N, (B,), dtype=torch.long)

    def recording(self):
        """The eager planning run: every draw inside the block is made as usual and its (B, N) noted in `plan`."""
        return ops.CTX.scoped(start_provider=self.record)

    def build(self):
        total = max(sum(b for b, _ in self.plan), 1)
        # two pinned staging buffers, used alternately: the host must not overwrite one while its
        # asynchronous copy to the device may still be pending (replays are not synchronised)
        self.host = [torch.empty(total, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.done = [None, None]
        self.turn = 0
        self.dev = torch.zeros(total, dtype=torch.int32, device=self.device)

    def refill(self):           # before every replay
        if not self.plan:
            return
        h = self.host[self.turn]
        if self.done[self.turn] is not None:
            self.done[self.turn].synchronize()
        off = 0
        for B, N in self.plan:
            h[off:off + B] = torch.randint(0, N, (B,), dtype=torch.long).to(torch.int32)
            off += B
        self.dev.copy_(h, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.done[self.turn] = ev
        self.turn ^= 1

    def provide(self, B, N):    # provider during capture
        off = sum(b for b, _ in self.plan[:self.cursor])
        assert self.cursor < len(self.plan) and self.plan[self.cursor] == (B, N), \
            'forward structure changed between planning and capture'
        self.cursor += 1
        return self.dev[off:off + B]

    @contextlib.contextmanager
    def providing(self):
        """The capture: the draws of the block are slices of the static buffer, in plan order.  A block that ends without
        an exception must have taken every planned draw -- one fewer would shift every later start of every replay."""
        self.cursor = 0
        with ops.CTX.scoped(start_provider=self.provide):
            yield
        if self.cursor != len(self.plan):
            raise RuntimeError('the captured forward drew %d FPS starts, the eager one %d' % (self.cursor, len(self.plan)))


class LRU(collections.OrderedDict):
    """An OrderedDict bounded to `limit` entries: get() marks an entry used, put() evicts the least recently used ones."""

    def __init__(self, limit, on_evict=None):
        super().__init__()
        self.limit, self.on_evict = limit, on_evict

    def get(self, k, default=None):
        if k in self:
            self.move_to_end(k)
            return self[k]
        return default

    def put(self, k, v):
        self[k] = v
        self.move_to_end(k)
        while len(self) > self.limit:
            _, old = self.popitem(last=False)
            if self.on_evict is not None:
                self.on_evict(old)
        return v


def refusal_text(exc):
    """The reason recorded for a refused capture: exception type and the first line of its message."""
    return '%s: %s' % (type(exc).__name__, str(exc).splitlines()[0] if str(exc) else '')


def tensor_outputs(out):
    """(outs, single): one tensor or a tuple of tensors (or None) as a list, and whether it was the single tensor."""
    single = isinstance(out, torch.Tensor)
    return ([out] if single else list(out if out is not None else ())), single
