"""CPU: the bookkeeping of the DGCNN prefix entry that also carries the forward values of the SA-node module's
pass-invariant half (proj, the residual layer's y and res, the residual BatchNorm's recorded statistics): the cache key,
liveness and copying.  The kernels behind it are held by tests/test_gpu_sa_shared.py."""
import copy

import torch

from sug_amd.model.Model import DGCNN
from sug_amd.model.model_utils import SharedHalf


def _entry(g, x):
    """An entry as DGCNN.forward stores it after a miss, on CPU stand-ins for the prefix tensors."""
    w = torch.ones(2, 8, 4, requires_grad=True)
    x1, x2 = w * 1.0, w * 2.0
    proj, y = x2[:, :, :3] * 3.0, x2 * 4.0
    res = y * 0.5
    bn = g.node_fea_adapt.residual.conv[1]
    shared = SharedHalf()
    assert not shared.filled
    shared.fill(proj, y, res, [(bn, torch.zeros(1, 5, 64))])
    assert shared.filled
    g._keep_prefix(x, x1, x2, shared, (torch.zeros(5, 64), torch.ones(5, 64)))
    return w, shared


def test_key_counts_the_versions_of_the_shared_half():
    g = DGCNN().train()
    x = torch.zeros(2, 3, 8, 1)
    ada = g.node_fea_adapt
    for p in (ada.pred_offset[0].weight, ada.residual.conv[0].weight, ada.residual.conv[0].bias, ada.residual.conv[1].weight,
              ada.residual.conv[1].bias, g.conv1.conv[0].weight, g.conv2.conv[1].weight):
        k0 = g._prefix_key(x)
        with torch.no_grad():
            p.add_(1.0)
        assert g._prefix_key(x) != k0
    k0 = g._prefix_key(x)
    with torch.no_grad():
        ada.trans.conv[0].weight.add_(1.0)          # not used by forward: not part of the key
        g.conv3.conv[0].weight.add_(1.0)            # behind the shared prefix
    assert g._prefix_key(x) == k0


def test_entry_shares_two_tensors_and_carries_the_half_as_values():
    g = DGCNN().train()
    x = torch.zeros(2, 3, 8, 1)
    _, shared = _entry(g, x)
    e = g.find_prefix(x)
    assert e is not None and e is g.last_prefix(x)
    assert len(e.tensors) == 2 and all(t.requires_grad for t in e.tensors)       # through autograd: x1, x2 only
    st1, st2, st_res, proj, y, res = e.extra
    assert proj is shared.proj and y is shared.y and res is shared.res and e.shared is shared
    for t in (proj, y, res):                                                     # values: no autograd history
        assert not t.requires_grad and t.grad_fn is None
    assert g.find_prefix(torch.zeros(2, 3, 8, 1)) is None           # another tensor object of the same shape
    with torch.no_grad():
        g.node_fea_adapt.residual.conv[0].weight.mul_(0.5)
    assert g.find_prefix(x) is None                                  # the weights moved on


def test_entry_without_a_recorded_half_still_shares_the_edgeconv_layers():
    g = DGCNN().train()
    x = torch.zeros(2, 3, 8, 1)
    w = torch.ones(2, 8, 4, requires_grad=True)
    g._keep_prefix(x, w * 1.0, w * 2.0, SharedHalf(), (torch.zeros(5, 64), torch.ones(5, 64)))
    e = g.find_prefix(x)
    assert e is not None and e.shared is None and e.extra[2:] == (None,) * 4


def test_entry_is_dead_after_a_backward():
    g = DGCNN().train()
    x = torch.zeros(2, 3, 8, 1)
    w, _ = _entry(g, x)
    e = g.find_prefix(x)
    assert e.alive and e.servable()
    e.tensors[1].sum().backward()
    assert w.grad is not None
    assert not e.alive and not e.servable()
    assert g.find_prefix(x) is None


def test_deepcopy_gets_a_dead_empty_entry():
    g = DGCNN().train()
    x = torch.zeros(2, 3, 8, 1)
    _entry(g, x)
    g2 = copy.deepcopy(g)
    assert g.find_prefix(x) is not None
    assert len(g2._prefix_cache) == 1
    for e in g2._prefix_cache.values():
        assert e.tensors == () and e.shared is None and not e.alive and not e.servable()
    assert g2.find_prefix(x) is None
    g2.clear_prefix_cache()
    assert g2._prefix_cache == {}
