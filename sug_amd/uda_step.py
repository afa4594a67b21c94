"""One two-phase training step of the PointDAN-style baselines, mirroring the batch loops of the reference's train_uda.py:149-184
(recipe 'uda') and train_dg_naive_mmd.py:225-263 (recipe 'naive_mmd') and their optimiser set-up (train_uda.py:101-113,
train_dg_naive_mmd.py:174-186):

  phase 1  heads of source and target -> a_s*(CE(s1) + CE(s2)) + a_t*(CE(t1) + CE(t2)) - discrepancy(t1, t2) -> backward ->
           optimizer_g.step(), optimizer_c.step(), both zeroed
  phase 2  ON THE UPDATED WEIGHTS: attention features of source and target -> mix_rbf_mmd2 ('uda') or mmd_cal(CLASS_MMD)
           ('naive_mmd') -> backward -> optimizer_dis.step(), zeroed

with `loss_total += loss_s.item() * data.size(0)` and its four companions (train_uda.py:180-184) kept on the device.

Two quirks of the reference survive because the loop is taken literally: the `pred_offset` parameters of the encoder are left out
of optimizer_g, so the gradient phase 1 gives them is not cleared by optimizer_g.zero_grad() and is applied, added to phase 2's, by
optimizer_dis; and the encoder's parameters keep separate Adam moments in optimizer_g and optimizer_dis.

Launch forms, as SourceStep: the step is a graph_replay.ReplayedStep, planned, captured (ONE graph: both phases, all three
updates, one stream) and replayed by that class's protocol.  With a plain nn.CrossEntropyLoss the scalar tail of phase 1 is
ops.mcd_loss (one launch each way, which also keeps four of the five books), with a model_utils.focal_loss (CLS_LOSS FocalLoss /
ClassWeighting of the shipped configurations) it is ops.cls_loss, which does the same; any other criterion, or fused_loss=False,
composes it from torch ops and keeps the books by in-place adds (`loss_form` says which ran).  Nothing waits for the device
until `epoch_totals()`.
`use_graph=False` launches the same ops eagerly: the graph's bit-for-bit twin.

What is shared "per step" elsewhere is per PHASE here, because the weights change in between: the 16-bit weight copies of the Point
Transformer's fp16 mode are refreshed at the start of each phase (phase 2: after the g / c update), the encoder's prefix cache and
the EdgeConv weight-split cache are dropped after each backward (both are keyed on the parameters' versions as well).
"""
import contextlib
import math

import torch
import torch.nn as nn

from . import ops
from .graph_replay import CriterionState, ReplayedStep, adam_choice, drop_weight_caches, hyper_key, plain_ce
from .model import mmd
from .train_step import discrepancy

CLASS_MMD = {'NAME': 'SOFT_MMD', 'LABEL_SCALE': 1.0}        # tools/cfgs/*/DG_baseline.yaml: METHODS.CLASS_MMD[0]
RECIPES = ('uda', 'naive_mmd')


def recipe_constants(recipe, src_weight=1.0, target_loss=0.0):
    """(a_s, a_t, r_s): loss = a_s*(CE(s1) + CE(s2)) + a_t*(CE(t1) + CE(t2)) - D, reported loss_s = r_s*(CE(s1) + CE(s2)).
    'uda' (train_uda.py:159-160): loss_s = CE1 + CE2, loss = weight*loss_s + loss_adv.  'naive_mmd'
    (train_dg_naive_mmd.py:234-241): loss_s = 0.5*CE1 + 0.5*CE2 and, with TARGET_LOSS > 0, loss = 0.5*SRC_LOSS_WEIGHT*loss_s +
    loss_adv + 0.5*TARGET_LOSS*loss_t, otherwise SRC_LOSS_WEIGHT*loss_s + loss_adv."""
    if recipe == 'uda':
        return float(src_weight), 0.0, 1.0
    if recipe == 'naive_mmd':
        if target_loss > 0:
            return 0.25 * float(src_weight), 0.25 * float(target_loss), 0.5
        return 0.5 * float(src_weight), 0.0, 0.5
    raise ValueError("UDAStep: recipe is 'uda' or 'naive_mmd' (got %r)" % (recipe,))


def _draw(B, N):
    return torch.randint(0, N, (B,), dtype=torch.long)


class UDAStep(ReplayedStep):
    def __init__(self, model, recipe='uda', lr=1e-3, weight_decay=5e-5, lr_scaler=1.0, src_weight=1.0, target_loss=0.0,
                 class_mmd=None, criterion=None, use_graph=True, fused_adam=None, fused_loss=True, pair_domains=True,
                 max_graphs=4):
        self.a_s, self.a_t, self.r_s = recipe_constants(recipe, src_weight, target_loss)
        self.model, self.recipe = model, recipe
        self.src_weight, self.target_loss = float(src_weight), float(target_loss)
        from .train_step import model_num_class, with_num_class
        self.num_class = model_num_class(model)         # the model's class count; the node term carries it (part of the graph key)
        self.class_mmd = with_num_class([class_mmd if class_mmd is not None else CLASS_MMD], self.num_class,
                                        'UDAStep: class_mmd')[0]
        self.base_lr, self.lr_scaler = float(lr), float(lr_scaler)
        self.c_lr = self.base_lr * 2 if recipe == 'uda' else self.base_lr           # train_uda.py:107 / train_dg_naive_mmd.py:179
        self.remain_epoch = 50 if recipe == 'uda' else 0                            # train_uda.py:99 / train_dg_naive_mmd.py:168
        self.criterion = criterion if criterion is not None else nn.CrossEntropyLoss()
        self.cons = 1.0             # GradReverse is the identity (model/Model.py:37-50): logged, never part of a graph key
        p0 = next(model.parameters())
        self.device = p0.device
        on_gpu = p0.is_cuda
        # a KPConv encoder is declined here with or without level caps: the two-phase step is not tested on the capacity form
        capturable = getattr(getattr(model, 'g', None), 'graph_capturable', True) and \
            not hasattr(getattr(model, 'g', None), 'set_level_caps')
        super().__init__(max_graphs, rows=2)
        self.use_graph = bool(use_graph) and on_gpu
        if self.use_graph and not capturable:           # Net_MDA('KPConv'): no static launch sequence, always eager
            self.use_graph = False
            self.why = '%s: level sizes depend on the data' % type(model.g).__name__ if getattr(model.g, 'level_caps', None) is None \
                else '%s: level caps are not supported by UDAStep (eager launches)' % type(model.g).__name__
        self.pair_domains = bool(pair_domains) and capturable and hasattr(model, 'forward_pair')
        # fused_loss=False is the plain composition throughout: the loss tail from torch ops and the heads' LayerNorm +
        # activation unfused, i.e. exactly what an unchanged caller's model(...) calls launch
        self.fused_loss = bool(fused_loss) and on_gpu
        AdamCls, kw = adam_choice(on_gpu, fused_adam, self.use_graph)
        params = [{'params': v} for k, v in model.g.named_parameters() if 'pred_offset' not in k]
        self.optimizer_g = AdamCls(params, lr=lr, weight_decay=weight_decay, **kw)
        self.optimizer_c = AdamCls([{'params': model.c1.parameters()}, {'params': model.c2.parameters()}], lr=self.c_lr,
                                   weight_decay=weight_decay, **kw)
        self.optimizer_dis = AdamCls([{'params': model.g.parameters()}, {'params': model.attention_s.parameters()},
                                      {'params': model.attention_t.parameters()}], lr=lr * lr_scaler, weight_decay=weight_decay,
                                     **kw)
        # the books of train_uda.py:130-135, :180-184: [loss_s*B, loss_adv*B, rows, target rows, loss_node*B]; the rows of steps
        # whose loss tail is composed are counted on the host (their number is known there)
        self._books = torch.zeros(5, dtype=torch.float64, device=self.device) if on_gpu else None
        self._w16_plans = [None, None]
        self._crit = CriterionState(max_graphs)         # the criterion by value, and the step's device copy of its alpha
        self.loss_form = None                           # phase 1's loss tail in the last step: 'mcd_loss' | 'cls_loss' | 'composed'
        self._split_layers = [m for m in model.modules() if hasattr(m, 'cache_weight_split')]

    def _opts(self):
        return (self.optimizer_g, self.optimizer_c, self.optimizer_dis)

    # ------------------------------------------------------------------ learning-rate schedules
    def set_epoch(self, epoch, max_epoch_num):
        """The learning rates at the start of `epoch` as the reference sets them: CosineAnnealingLR(T_max = max_epoch_num + 50
        for 'uda', max_epoch_num for 'naive_mmd'; eta_min = 0) stepped with an explicit epoch (= its closed form) for optimizer_g
        and optimizer_c, utils/train_utils.py:39-48 `adjust_learning_rate` for optimizer_dis (halved every 5 epochs up to epoch
        30, every 10 afterwards; untouched at epoch 0).  Returns (lr_g, lr_c, lr_dis, cons), cons = sin((epoch + 1) /
        max_epoch_num * pi / 2) for logging."""
        cos = (1.0 + math.cos(math.pi * epoch / (max_epoch_num + self.remain_epoch))) / 2.0
        for opt, base in ((self.optimizer_g, self.base_lr), (self.optimizer_c, self.c_lr)):
            for g in opt.param_groups:
                g['lr'] = base * cos
        if epoch > 0:
            lr = self.base_lr * self.lr_scaler * (0.5 ** (epoch // 5 if epoch <= 30 else epoch // 10))
            for g in self.optimizer_dis.param_groups:
                g['lr'] = lr
        self.cons = math.sin((epoch + 1) / max_epoch_num * math.pi / 2)
        return (self.optimizer_g.param_groups[0]['lr'], self.optimizer_c.param_groups[0]['lr'],
                self.optimizer_dis.param_groups[0]['lr'], self.cons)

    # ------------------------------------------------------------------ the epoch's books
    def epoch_totals(self, reset=True):
        """(loss_total, loss_adv_total, loss_node_total, data_total, data_t_total) since the last reset, as Python floats: the one
        host read of an epoch (train_uda.py:186-190 prints the first three over data_total every ten batches)."""
        if self._books is None:
            return 0.0, 0.0, 0.0, 0.0, 0.0
        from .train_step import check_level_caps
        check_level_caps(getattr(self.model, 'g', None), reset)     # a KPConv encoder run eagerly with level caps: overflow raises
        ls, adv, rows, rows_t, node = self._books.tolist()
        rows += self._rows_host[0]
        rows_t += self._rows_host[1]
        if reset:
            self._books.zero_()
            self._rows_host[:] = (0, 0)
        return float(ls), float(adv), float(node), float(rows), float(rows_t)

    # ------------------------------------------------------------------ step
    def step(self, data, label, data_t, label_t):
        """data, data_t [B,3,N,1] fp32, label, label_t [B] int64, all on the HIP device -> (loss_s, loss_adv, loss_node) as 0-d
        device tensors of the caller's own (a replay does not overwrite them).  No host wait."""
        ops._need_gpu(data, label, data_t, label_t, next(self.model.parameters()))
        for x, y in ((data, label), (data_t, label_t)):
            if x.dim() != 4 or x.shape[0] != y.shape[0] or y.dtype != torch.int64:
                raise RuntimeError('UDAStep.step: clouds [B,3,N,1] and labels int64 [B] (got %s, %s %s)' %
                                   (tuple(x.shape), tuple(y.shape), y.dtype))
        if self.use_graph:
            return self._graph_step((data, label, data_t, label_t))
        return self._eager_step(data, label, data_t, label_t)

    def _graph_key(self, batch):
        """Everything a captured step bakes in by value (`cons` is not: GradReverse is the identity)."""
        from .model import Ptran_transformer as PT
        c = self.criterion
        crit = ('ce', int(c.ignore_index)) if plain_ce(c) else (self._crit.record(c, self.max_graphs) or ('call', id(c), repr(c)))
        hyp = tuple(hyper_key(o) for o in self._opts())
        return (tuple(tuple(t.shape) for t in batch), self.recipe, self.a_s, self.a_t, self.r_s, self.src_weight, self.target_loss,
                repr(sorted(self.class_mmd.items())), crit, self.model.training, self.fused_loss, self.pair_domains,
                PT.GEMM_DTYPE, getattr(PT, 'PROJ_16BIT', None), hyp)

    @contextlib.contextmanager
    def _step_scope(self):
        """The forwards of one step: a start provider is in force (the graph's feeder, or the plain CPU-generator draw), so
        that the model's per-call graphs (sug_amd.call_graphs, keyed on ops.CTX.unscoped()) decline -- the step owns the launch
        form; the fused LayerNorm + activation of the heads unless fused_loss=False."""
        fields = {'fused_heads': self.fused_loss or ops.CTX.fused_heads}
        if ops.CTX.start_provider is None:
            fields['start_provider'] = _draw
        with ops.CTX.scoped(**fields):
            yield

    @contextlib.contextmanager
    def _phase_scope(self, phase):
        """The forwards of one PHASE: 16-bit weight copies (Point Transformer, fp16 mode) made from the weights as they are
        NOW -- from the second step on by one multi-tensor copy into the first step's buffers -- and every num_batches_tracked
        increment in one launch."""
        with ops.w16_scope(self._w16_plans, phase), ops.deferred_bn_counts():
            yield

    def _after_backward(self):
        """Nothing computed from the weights outlives the update that follows."""
        drop_weight_caches(self.model, self._split_layers, hasattr(self.model.g, 'clear_prefix_cache'))

    def _cls_loss_tail(self, rec, ys1, ys2, yt1, yt2, label):
        """Phase 1's loss for a recognised criterion other than the plain cross entropy as ops.cls_loss (a_d = 1: the
        discrepancy enters as it is), books included; None where the kernel does not take it."""
        if ys1.dim() != 2 or (rec.alpha is not None and len(rec.alpha) < ys1.shape[1]):
            return None
        label_t = label if self.a_t else None               # (the target rows are scored against the SOURCE labels)
        alpha = self._crit.alpha_on(rec, ys1.device)
        if not ops.cls_loss_supported(ys1, ys2, yt1, yt2, label, label_t, alpha, rec.gamma, rec.reduction, self.a_t):
            return None
        self.loss_form = 'cls_loss'
        return ops.cls_loss(ys1, ys2, yt1, yt2, label, label_t, alpha, rec.gamma, rec.reduction, rec.ignore_index, self.a_s,
                            self.a_t, 1.0, self.r_s, totals=self._books[:4])

    def _eager_step(self, data, label, data_t, label_t):
        model, B, Bt = self.model, data.shape[0], data_t.shape[0]
        pair = None
        if self.pair_domains and data.shape == data_t.shape and model.training:
            pair = torch.cat((data, data_t), dim=0)
        with self._step_scope():
            # ---- phase 1 (train_uda.py:149-166)
            fused = self.fused_loss and plain_ce(self.criterion)
            rec = self._crit.record(self.criterion, self.max_graphs) if (self.fused_loss and not fused) else None
            out = None
            self.loss_form = 'composed'
            with self._phase_scope(0):
                if pair is not None:
                    y1, y2, _, _ = model.forward_pair(pair, paired_out=True)
                    if fused and ops.mcd_loss_supported(y1, y2, None, None, label, self.a_t):
                        out = ops.mcd_loss(y1, y2, None, None, label, label if self.a_t else None, self.a_s, self.a_t, self.r_s,
                                           totals=self._books[:4])
                        self.loss_form = 'mcd_loss'
                    elif rec is not None:
                        out = self._cls_loss_tail(rec, y1, y2, None, None, label)
                    if out is None:
                        (pred_s1, pred_t1), (pred_s2, pred_t2) = ops.split_halves(y1), ops.split_halves(y2)
                else:
                    pred_s1, pred_s2 = model(data)
                    pred_t1, pred_t2 = model(data_t, constant=self.cons, adaptation=True)
                    if fused and ops.mcd_loss_supported(pred_s1, pred_s2, pred_t1, pred_t2, label, self.a_t):
                        # (the target rows are scored against the SOURCE labels, train_dg_naive_mmd.py:236-237)
                        out = ops.mcd_loss(pred_s1, pred_s2, pred_t1, pred_t2, label, label if self.a_t else None, self.a_s,
                                           self.a_t, self.r_s, totals=self._books[:4])
                        self.loss_form = 'mcd_loss'
                    elif rec is not None:
                        out = self._cls_loss_tail(rec, pred_s1, pred_s2, pred_t1, pred_t2, label)
            if out is not None:
                loss, loss_s, loss_adv = out[0], out[1], out[2]
            else:
                crit = self.criterion
                loss_s1, loss_s2 = crit(pred_s1, label), crit(pred_s2, label)
                loss_adv = - 1 * discrepancy(pred_t1, pred_t2)
                if self.recipe == 'uda':
                    loss_s = loss_s1 + loss_s2
                    loss = self.src_weight * loss_s + loss_adv
                else:
                    loss_s = 0.5 * loss_s1 + 0.5 * loss_s2
                    if self.target_loss > 0:
                        loss_t = 0.5 * crit(pred_t1, label) + 0.5 * crit(pred_t2, label)
                        loss = 0.5 * self.src_weight * loss_s + loss_adv + 0.5 * self.target_loss * loss_t
                    else:
                        loss = self.src_weight * loss_s + loss_adv
                with torch.no_grad():                       # loss_total += loss_s * B; loss_adv_total += loss_adv * B, in fp64
                    self._books[0:1].add_(loss_s.detach().reshape(1), alpha=B)
                    self._books[1:2].add_(loss_adv.detach().reshape(1), alpha=B)
                self._rows_host[0] += B
                self._rows_host[1] += Bt
            loss.backward()
            self._after_backward()
            self.optimizer_g.step()
            self.optimizer_c.step()
            self.optimizer_g.zero_grad()        # (not the pred_offset parameters: their gradient waits for optimizer_dis)
            self.optimizer_c.zero_grad()
            # ---- phase 2, on the updated weights (train_uda.py:169-178)
            with self._phase_scope(1):
                if pair is not None:
                    node_s, node_t = model.forward_pair(pair, node_adaptation=True)
                else:
                    node_s = model(data, node_adaptation_s=True)
                    node_t = model(data_t, node_adaptation_t=True)
            if self.recipe == 'uda':
                loss_node = mmd.mix_rbf_mmd2(node_s, node_t, mmd.sigma_list)
            else:
                loss_node = mmd.mmd_cal(label, node_s, label_t, node_t, self.class_mmd)
            loss_node.backward()
            self._after_backward()
            ops.clear_rows_cache()
            self.optimizer_dis.step()
            self.optimizer_dis.zero_grad()
            with torch.no_grad():                           # loss_node_total += loss_node * B
                self._books[4:5].add_(loss_node.detach().reshape(1), alpha=B)
        return loss_s.detach(), loss_adv.detach(), loss_node.detach()
