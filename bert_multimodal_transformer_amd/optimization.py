"""AdamW + get_linear_schedule_with_warmup -- the transformers==3.0.2 API the reference imports
(/root/reference/multimodal_driver.py:27-28, 345-350), running on the fused HIP kernel (csrc/adamw.hip).

    optimizer = AdamW(optimizer_grouped_parameters, lr=args.learning_rate)
    scheduler = get_linear_schedule_with_warmup(optimizer, num_warmup_steps=..., num_training_steps=...)

Parameters that are views of a model's flat buffer (bert.py) are updated with ONE launch per param group over the
contiguous flat range (m, v live in flat buffers too; the bf16 operand shadow is refreshed and the gradient cleared
in the same pass); any other CUDA tensor gets one launch per tensor.  Formula: see oracle/optim_ref.py -- eps 1e-6
outside the sqrt, bias correction folded into step_size, decoupled decay AFTER the update.

AdamW(..., max_grad_norm=x) clips the global gradient norm as torch.nn.utils.clip_grad_norm_(parameters, x) would in front of
step(), without scaling any gradient: one HIP pass reads the flat gradient range (csrc/gradnorm.hip), and the coefficient goes into the
gradient scale of the update kernels.  Inside the single-call step (model.train_step) no host sync is involved; step() itself reads
the coefficient back once.
"""
import math
import os

import numpy as np
import torch

from . import _lib

# limits of the engines' update-class table and segment map (include/magbert_hip.h)
UPDATE_CLASSES_MAX = 32
UPDATE_SEGMENTS_MAX = 128


def _distrust_word_moments(core):
    """the Adam moments of `core`'s flat buffer are about to be written from here (bert._Core.distrust_word_moments: the engine's single-call
    step keeps a proof about the word rows whose moments are zero; new moment tensors it notices itself, by their address)"""
    fn = getattr(core, "distrust_word_moments", None)
    if fn is not None:
        fn()


FROZEN = -1          # the class plan_*_segments(..., frozen=True) gives a segment no parameter group holds


def plan_update_segments(tensors, group_of_tensor, n_update_end, frozen=False):
    """The segment map of a classed single-call step (include/magbert_hip.h: mb_*_set_update_map), from the flat layout alone.

    tensors: the layout's table, (name, offset, numel, ...) per tensor (_Core.tensors); group_of_tensor: per tensor the index of the
    one parameter group that holds it, None for a tensor no group holds, or a collection of indices when several do; tensors at or
    behind n_update_end (frozen slots) are not looked at.  Returns (boundaries, classes): segment s = [boundaries[s],
    boundaries[s + 1]) -- a maximal run of consecutive tensors of one group, the alignment gap behind a tensor included -- belongs to
    group classes[s]; boundaries are tensor offsets, from 0 to n_update_end.  None when a tensor below n_update_end is not in
    exactly one group, the tensors do not tile [0, n_update_end), or there are more than UPDATE_CLASSES_MAX groups or
    UPDATE_SEGMENTS_MAX segments.

    frozen=True: a tensor no group holds (None, or an empty collection) is frozen, not a reason to decline.  A maximal run of consecutive
    frozen tensors is a segment of class FROZEN, and the result is (boundaries, classes, frozen_flags) with one 0 / 1 flag per segment
    (include/magbert_hip.h: mb_*_set_update_frozen).  Frozen segments count towards UPDATE_SEGMENTS_MAX, FROZEN is no class; None when
    every tensor is frozen."""
    if len(tensors) != len(group_of_tensor):
        return None
    rows = sorted((int(t[1]), int(t[2]), g) for t, g in zip(tensors, group_of_tensor) if int(t[1]) < n_update_end)
    boundaries, classes = [], []
    cursor = 0
    for off, numel, g in rows:
        if isinstance(g, (list, tuple, set, frozenset)):
            if len(g) > 1 or (len(g) == 0 and not frozen):
                return None
            g = next(iter(g)) if g else None
        if g is None and frozen:
            g = FROZEN
        elif g is not None and frozen and int(g) < 0:
            return None
        if g is None or off != cursor or numel < 1:
            return None
        cursor = (off + numel + 63) // 64 * 64          # tensors are 64-float aligned in the flat layout
        if not classes or classes[-1] != g:
            boundaries.append(off)
            classes.append(int(g))
    if cursor != n_update_end or not classes:
        return None
    boundaries.append(int(n_update_end))
    real = set(classes) - ({FROZEN} if frozen else set())
    if not real or len(real) > UPDATE_CLASSES_MAX or len(classes) > UPDATE_SEGMENTS_MAX:
        return None
    if frozen:
        return boundaries, classes, [1 if c == FROZEN else 0 for c in classes]
    return boundaries, classes


def pair_update_groups(hyper, hints=None):
    """Which parameter groups may share an update class (include/magbert_hip.h: mb_*_set_update_decay).

    hyper: per group (lr, betas, eps, correct_bias, weight_decay).  Two groups pair when lr, betas, eps and correct_bias are equal and
    one of them has weight_decay == 0: the class carries the other's weight_decay, and the zero-decay group's segments are marked
    no-decay.  hints (optional, one value per group, None = no hint) only choose among several possible partners: a decaying group
    takes the first zero-decay group of its (lr, betas, eps, correct_bias) that has its hint, and what is left pairs in index order.
    AdamW hands over the groups' initial_lr: during a warm-up from lr 0 every group has the same lr, and pairs made by index alone
    would break -- and be planned again -- at the next step.  A group without a partner stays a class of its own.  Returns
    (class_of_group, no_decay_of_group, members): class ids are dense, numbered by the smallest group index of the class; members[c] =
    (the group whose values the class carries, its zero-decay partner or None)."""
    decaying, zero = {}, {}
    for g, (lr, betas, eps, correct_bias, wd) in enumerate(hyper):
        key = (float(lr), tuple(float(b) for b in betas), float(eps), bool(correct_bias))
        (zero if float(wd) == 0.0 else decaying).setdefault(key, []).append(g)
    partner = {}
    for key, gs in decaying.items():
        free = list(zero.get(key, []))
        if hints is not None:
            for g in gs:
                z = next((z for z in free if hints[g] is not None and hints[z] == hints[g]), None)
                if z is not None:
                    partner[g], partner[z] = z, g
                    free.remove(z)
        for g, z in zip([g for g in gs if g not in partner], free):
            partner[g], partner[z] = z, g
    class_of, no_decay, members = [None] * len(hyper), [False] * len(hyper), []
    for g in range(len(hyper)):
        if class_of[g] is not None:
            continue
        class_of[g] = len(members)
        other = partner.get(g)
        if other is None:
            members.append((g, None))
            continue
        class_of[other] = len(members)
        carrier, z = (other, g) if float(hyper[g][4]) == 0.0 else (g, other)
        no_decay[z] = True
        members.append((carrier, z))
    return class_of, no_decay, members


def plan_paired_segments(tensors, group_of_tensor, n_update_end, class_of_group, no_decay_of_group, frozen=False):
    """plan_update_segments over the classes of paired groups (pair_update_groups): (boundaries, classes, no_decay_flags).  A segment
    is a maximal run of consecutive tensors of one class AND one flag -- the decayed and the undecayed tensors of a class that touch
    are two segments -- and flag s is 1 where segment s holds a zero-decay partner's tensors.  None under plan_update_segments' own
    conditions, with the classes counted after pairing.  frozen=True, as there: tensors no group holds become segments of class FROZEN
    (no-decay flag 0), and the result is (boundaries, classes, no_decay_flags, frozen_flags)."""
    if len(tensors) != len(group_of_tensor):
        return None
    rows = sorted((int(t[1]), int(t[2]), g) for t, g in zip(tensors, group_of_tensor) if int(t[1]) < n_update_end)
    boundaries, classes, flags = [], [], []
    cursor = 0
    for off, numel, g in rows:
        if isinstance(g, (list, tuple, set, frozenset)):
            if len(g) > 1 or (len(g) == 0 and not frozen):
                return None
            g = next(iter(g)) if g else None
        if off != cursor or numel < 1:
            return None
        if g is None and frozen:
            c, f = FROZEN, 0
        elif g is None or not 0 <= int(g) < len(class_of_group):
            return None
        else:
            c, f = int(class_of_group[int(g)]), 1 if no_decay_of_group[int(g)] else 0
        cursor = (off + numel + 63) // 64 * 64          # tensors are 64-float aligned in the flat layout
        if not classes or classes[-1] != c or flags[-1] != f:
            boundaries.append(off)
            classes.append(c)
            flags.append(f)
    if cursor != n_update_end or not classes:
        return None
    boundaries.append(int(n_update_end))
    real = set(classes) - ({FROZEN} if frozen else set())
    if not real or len(real) > UPDATE_CLASSES_MAX or len(classes) > UPDATE_SEGMENTS_MAX:
        return None
    if frozen:
        return boundaries, classes, flags, [1 if c == FROZEN else 0 for c in classes]
    return boundaries, classes, flags


_NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")          # multimodal_driver.py:336
_HEAD_MARKS = ("MAG.", "pooler.", "classifier.", "sequence_summary.", "logits_proj.")


def _depth_of(name, num_layers):
    """0 = embeddings (and any other encoder parameter), l + 1 = layer l, num_layers + 1 = the new parameters (MAG, pooler, heads)"""
    for mark in ("encoder.layer.", "transformer.layer."):
        at = name.find(mark)
        if at >= 0:
            return int(name[at + len(mark):].split(".")[0]) + 1
    if any(name.startswith(mk) or ("." + mk) in name for mk in _HEAD_MARKS):
        return num_layers + 1
    return 0


def layerwise_lr_groups(named_parameters, num_layers, lr, layer_decay=1.0, head_lr=None, weight_decay=0.01):
    """Parameter groups for AdamW with layer-wise learning-rate decay and / or a learning rate of their own for the new parameters.

    named_parameters: (name, parameter) pairs.  Depth 0 = the embeddings, depth l + 1 = `encoder.layer.l.` (BERT) / `transformer.layer.l.`
    (XLNet, its per-layer relative-attention biases included), any other encoder parameter goes with the embeddings; parameters whose
    requires_grad is false (model.freeze) are in no group; depth d trains at
    lr * layer_decay ** (num_layers + 1 - d).  The new parameters -- MAG.*, the pooler, classifier, sequence_summary, logits_proj --
    train at head_lr (lr when None).  Every learning rate is split by the reference's no-decay rule (multimodal_driver.py:336: bias,
    LayerNorm.bias, LayerNorm.weight in the name); empty groups are dropped.  With layer_decay == 1.0 and head_lr None the result is
    exactly multimodal_driver.optimizer_grouped_parameters(): two groups without an lr of their own."""
    everything = list(named_parameters)
    named = [(n, p) for n, p in everything if getattr(p, "requires_grad", True)]          # frozen parameters (model.freeze) are in no group
    is_nd = lambda n: any(nd in n for nd in _NO_DECAY)
    if layer_decay == 1.0 and head_lr is None:
        two = [{"params": [p for n, p in named if not is_nd(n)], "weight_decay": weight_decay},
               {"params": [p for n, p in named if is_nd(n)], "weight_decay": 0.0}]
        # (with nothing frozen: the two groups as ever, even an empty one; a group that freezing emptied is left out)
        return two if len(named) == len(everything) else [g for g in two if g["params"]]
    buckets = {}
    for n, p in named:
        d = _depth_of(n, num_layers)
        if d < 0 or d > num_layers + 1:
            raise ValueError("parameter %s names layer %d of a model of %d layers" % (n, d - 1, num_layers))
        buckets.setdefault((d, is_nd(n)), []).append(p)
    groups = []
    for d in range(num_layers + 2):
        if d == num_layers + 1:
            lr_d = lr if head_lr is None else head_lr
        else:
            lr_d = lr * layer_decay ** (num_layers + 1 - d)
        for nd in (False, True):
            if buckets.get((d, nd)):
                groups.append({"params": buckets[(d, nd)], "weight_decay": 0.0 if nd else weight_decay, "lr": lr_d})
    return groups


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: {}".format(betas))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias)
        super().__init__(params, defaults)
        self.grad_scale = 1.0          # data parallel: 1/world_size when gradients were SUM-reduced
        # global gradient-norm clipping (None, <= 0 or non-finite: off).  The norm is that of the gradient as the update sees it
        # (grad_scale included) over every parameter of this optimizer; may be changed between steps.
        self.max_grad_norm = max_grad_norm
        self._clip_last = None         # where the last update left (norm, coef): a core (single-call step) or the two floats
        self.fused_zero_grad = True    # clear gradients inside the update kernel (zero_grad() then costs nothing)
        self._plan = None
        self._class_frozen = {}        # per flat buffer: the frozen flags of that map's segments (tensors no group holds), or None
        self._class_maps = {}          # per flat buffer: the segment map of a classed single-call step (flat_step_args), or None
        self._t = 0
        self._dp = None              # set by distributed.DataParallel

    def _clip_value(self):
        """max_grad_norm as the engine takes it: a float > 0, or 0.0 for off"""
        x = self.max_grad_norm
        if x is None:
            return 0.0
        x = float(x)
        return x if (math.isfinite(x) and x > 0.0) else 0.0

    @property
    def last_grad_norm(self):
        """the gradient norm the last clipped update measured (before clipping), None when no such update has run.  Read from the
        device when asked for, not on every step."""
        rec = self.last_grad_clip
        return None if rec is None else rec[0]

    @property
    def last_grad_clip(self):
        """(norm, coef) of the last clipped update, or None"""
        if self._clip_last is None:
            return None
        if isinstance(self._clip_last, tuple):
            return self._clip_last
        return self._clip_last.grad_clip_stats()

    def _clip_coef(self, L):
        """step() with max_grad_norm: (norm, coef) over everything this optimizer is about to update.  The usual case -- one
        contiguous flat range of one model, no loose tensor with a gradient -- is ONE mb_grad_clip_coef call whose coefficient is the
        float the single-call step forms on the device.  Otherwise the pieces' norms (one call per contiguous flat range; loose
        tensors with torch, in double) are combined on the host."""
        max_norm = self._clip_value()
        ranges = {}
        for it in self._plan:
            if it[0] == "flat":
                ranges.setdefault(id(it[2]), (it[2], []))[1].append((it[3], it[4]))
        pieces = []
        for core, sp in ranges.values():
            sp.sort()
            merged = []
            for a, b in sp:
                if merged and a <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], b)
                elif b > a:
                    merged.append([a, b])
            pieces += [(core, a, b) for a, b in merged]
        loose = [it[2] for it in self._plan if it[0] != "flat" and it[2].grad is not None]

        def call(core, a, b, sumsq=False):
            n = b - a
            need = L.mb_grad_clip_scratch_bytes(n)
            scratch = getattr(core, "_clip_scratch", None)
            if scratch is None or scratch.numel() * 8 < need:
                scratch = core._clip_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=core.grads.device)
                core._clip_out = torch.empty(2, dtype=torch.float32, device=core.grads.device)
            _lib.check(L.mb_grad_clip_coef(core.grads.data_ptr() + 4 * a, n, max_norm, self.grad_scale, scratch.data_ptr(),
                                           core._clip_out.data_ptr(), core.stream()))
            if sumsq:       # the piece's sum of squares in double: the launch's per-block partials are still in the scratch
                return float(scratch[: need // 8].sum())
            norm, coef = core._clip_out.cpu().tolist()          # the one host sync of this path
            return norm, coef

        if len(pieces) == 1 and not loose:
            return call(*pieces[0])
        # Several pieces (frozen tensors between them): their sums of squares are combined in double and the coefficient is formed as
        # grad_clip_finalize forms it -- norm = grad_scale * sqrt(sum), coef = (float)min(1, (double)max_norm / (norm + 1e-6)) -- so
        # it is the float the single-call step computes over the same pieces unless the two double sums, which differ in summation
        # order only, straddle a rounding boundary of that float.  (Piece norms rounded to float each lost that: 7e-8 relative.)
        total = 0.0
        for piece in pieces:
            total += call(*piece, sumsq=True)
        for p in loose:
            total += float(p.grad.detach().double().pow(2).sum())
        norm = float(np.float32(self.grad_scale)) * math.sqrt(total)
        c = float(np.float32(max_norm)) / (norm + 1e-6)
        return norm, float(np.float32(1.0 if c > 1.0 else c))

    # -- planning: map groups onto contiguous flat ranges ------------------------------------------------
    def _build_plan(self):
        plan = []
        for gi, group in enumerate(self.param_groups):
            flat, loose = {}, []
            for p in group["params"]:
                info = getattr(p, "_mb_flat", None)
                if info is None:
                    loose.append(p)
                else:
                    core, off, numel, _ = info
                    flat.setdefault(id(core), (core, []))[1].append((off, numel))
            for core, spans in flat.values():
                spans.sort()
                merged = []
                for off, numel in spans:
                    end = (off + numel + 63) // 64 * 64          # tensors are 64-float aligned in the flat layout
                    if merged and off <= merged[-1][1]:
                        merged[-1][1] = max(merged[-1][1], end)
                    else:
                        merged.append([off, end])
                if not hasattr(core, "_adam_m"):
                    core._adam_m = torch.zeros_like(core.params)
                    core._adam_v = torch.zeros_like(core.params)
                for a, b in merged:
                    plan.append(("flat", gi, core, a, min(b, core.n_params)))
            for p in loose:
                plan.append(("loose", gi, p))
        self._plan = plan
        # cores whose GEMM-weight range [sh_begin, sh_end) is updated -- hence zeroed -- entirely by this optimizer: after a
        # fused step their layer weight gradients are known to be zero (mb_bert_mark_grads_zero: the next backward stores them)
        self._covers = {}
        spans = {}
        for it in plan:
            if it[0] == "flat":
                spans.setdefault(id(it[2]), (it[2], []))[1].append((it[3], it[4]))
        for cid, (core, sp) in spans.items():
            sp.sort()
            reach = core.sh_begin
            for a, b in sp:
                if a <= reach:
                    reach = max(reach, b)
            self._covers[cid] = (core, reach >= core.sh_end)

    def _mark_zero(self):
        for core, covered in self._covers.values():
            if covered:
                core.mark_grads_zero(True)

    @staticmethod
    def _hyper(group):
        return (group["lr"], group["betas"], group["eps"], group["correct_bias"], group["weight_decay"])

    def _pairs_hold(self, partners):
        """the paired groups of a cached map still agree on lr / betas / eps / correct_bias, and the zero side is still zero"""
        for g, z in partners:
            if z is None:
                continue
            a, b = self._hyper(self.param_groups[g]), self._hyper(self.param_groups[z])
            if float(a[0]) != float(b[0]) or tuple(a[1]) != tuple(b[1]) or float(a[2]) != float(b[2]) or bool(a[3]) != bool(b[3]) or float(b[4]) != 0.0:
                return False
        return True

    def _class_map(self, core):
        """(boundaries, classes, groups, no_decay, partners) of this optimizer's groups over `core`'s flat layout -- the segment map of a
        classed step and the parameter group behind every class -- or None.  plan_update_segments comes first: every set of groups it
        takes gets the map it always got, with no_decay = None.  Only when it declines are the groups paired (pair_update_groups,
        plan_paired_segments): classes then stand for up to two groups, groups[c] is the one whose values class c carries, partners[c]
        = (that group, its zero-decay partner or None), and no_decay marks the partner's segments.  The plan is computed once;
        flat_step_args drops it when a pair no longer holds.  Tensors no group holds are frozen: _class_frozen keeps one flag per
        segment for them (1 = frozen; None when every tensor has a group)."""
        if id(core) not in self._class_maps:
            owner = {}
            for gi, group in enumerate(self.param_groups):
                for p in group["params"]:
                    info = getattr(p, "_mb_flat", None)
                    if info is not None and info[0] is core:
                        owner.setdefault(info[1], set()).add(gi)
            n_end = getattr(core, "n_update_end", core.n_params)
            # tensors no group holds are frozen (model.freeze + groups built from requires_grad): segments of their own, marked, whose
            # class is not looked at (they carry class 0)
            owners = [owner.get(t[1]) for t in core.tensors]
            planned = plan_update_segments(core.tensors, owners, n_end, frozen=True)
            if planned is not None:
                groups = sorted(set(planned[1]) - {FROZEN})
                self._class_frozen[id(core)] = planned[2] if any(planned[2]) else None
                planned = (planned[0], [0 if g == FROZEN else groups.index(g) for g in planned[1]], groups, None, [(g, None) for g in groups])
            else:
                class_of, no_decay, members = pair_update_groups([self._hyper(g) for g in self.param_groups],
                                                                 hints=[g.get("initial_lr") for g in self.param_groups])
                paired = plan_paired_segments(core.tensors, owners, n_end, class_of, no_decay, frozen=True)
                if paired is not None:
                    used = sorted(set(paired[1]) - {FROZEN})          # (groups without a tensor in this buffer leave holes in the class ids)
                    planned = (paired[0], [0 if c == FROZEN else used.index(c) for c in paired[1]], [members[c][0] for c in used], paired[2],
                               [members[c] for c in used])
                    self._class_frozen[id(core)] = paired[3] if any(paired[3]) else None
            self._class_maps[id(core)] = planned
        return self._class_maps[id(core)]

    def flat_step_args(self, core, allow_dp=False):
        """Hyper-parameters of step() as ONE whole-buffer update.  When this optimizer is exactly the driver's two parameter groups
        (multimodal_driver.py:329-343) over `core`'s flat buffer -- [0, n_decay) decayed, the rest not, same lr / betas / eps / bias
        correction in both -- the scalars of that update.  For any other set of groups that covers the buffer's trainable range exactly
        once: the same dictionary with "map" = (boundaries, classes), the segment map (plan_update_segments), and "classes" = the
        per-class lists lr / beta1 / beta2 / eps / weight_decay / correct_bias of this step (include/magbert_hip.h:
        mb_*_set_update_map / _set_update_values).  More groups than the class table holds are paired first (_class_map): the
        dictionary then also carries "no_decay", one flag per segment (mb_*_set_update_decay), and a class's values are those of the
        pair's decaying group.  A cached pairing is checked on every call -- a pair whose groups no longer agree is planned again, which
        may end in None.  Either dictionary carries "max_grad_norm" (0.0 = no clipping), which the step installs
        with mb_*_set_grad_clip; under allow_dp a clipping optimizer gets None -- the data-parallel single call has no norm of the reduced
        gradient, so that step is driven from Python.  Tensors of the buffer that no group holds are frozen: the map then has segments
        of their own for them and the dictionary carries "frozen", one flag per segment (mb_*_set_update_frozen) -- the step leaves
        their parameters, moments and shadow alone and skips the launches that only they need.  None otherwise (loose tensors with gradients, a partly covered buffer, more groups or
        segments than the engine takes, fused_zero_grad off, data parallel -- whose step keeps its Python-driven exchange for classed
        optimizers, allow_dp or not): the caller then runs step() as usual.  Used by the whole-step graph (mb_bert_train_step), which
        applies the update itself."""
        if (self._dp is not None and not allow_dp) or not self.fused_zero_grad:
            return None
        if allow_dp and self._clip_value() > 0.0:
            return None
        if self._plan is None:
            self._build_plan()
        flats = [it for it in self._plan if it[0] == "flat"]
        loose = [it for it in self._plan if it[0] != "flat"]
        if any(it[2].grad is not None for it in loose):           # grad-less parameters (MAG-XLNet's frozen mask_emb) are skipped by step() too
            return None
        two = self._two_group_args(core, flats)
        if two is not None or self._dp is not None or not flats or any(it[2] is not core for it in flats):
            if two is not None:
                two["max_grad_norm"] = self._clip_value()
            return two
        planned = self._class_map(core)
        if planned is not None and not self._pairs_hold(planned[4]):
            del self._class_maps[id(core)]          # a pair was broken by hand: pair and plan again with the groups as they are now
            planned = self._class_map(core)
        if planned is None:
            return None
        boundaries, classes, groups, no_decay, _ = planned
        frozen = self._class_frozen.get(id(core))
        gs = [self.param_groups[g] for g in groups]
        marks = {} if no_decay is None else {"no_decay": list(no_decay)}
        if frozen is not None:
            marks["frozen"] = list(frozen)
        return dict(m=core._adam_m, v=core._adam_v, grad_scale=float(self.grad_scale), map=(boundaries, classes),
                    max_grad_norm=self._clip_value(), **marks,
                    classes=dict(lr=[float(g["lr"]) for g in gs], beta1=[float(g["betas"][0]) for g in gs],
                                 beta2=[float(g["betas"][1]) for g in gs], eps=[float(g["eps"]) for g in gs],
                                 weight_decay=[float(g["weight_decay"]) for g in gs],
                                 correct_bias=[1 if g["correct_bias"] else 0 for g in gs]))

    def _two_group_args(self, core, flats):
        if len(flats) != 2 or any(it[2] is not core for it in flats):
            return None
        (_, g0, _, a0, b0), (_, g1, _, a1, b1) = sorted(flats, key=lambda it: it[3])
        if (a0, b0, a1, b1) != (0, core.n_decay, core.n_decay, getattr(core, "n_update_end", core.n_params)):
            return None
        ga, gb = self.param_groups[g0], self.param_groups[g1]
        if any(ga[k] != gb[k] for k in ("lr", "betas", "eps", "correct_bias")) or gb["weight_decay"] != 0.0:
            return None
        return dict(m=core._adam_m, v=core._adam_v, lr=float(ga["lr"]), beta1=float(ga["betas"][0]), beta2=float(ga["betas"][1]),
                    eps=float(ga["eps"]), weight_decay=float(ga["weight_decay"]), correct_bias=bool(ga["correct_bias"]),
                    grad_scale=float(self.grad_scale))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._plan is None:
            self._build_plan()
        L = _lib.lib()
        self._t += 1
        for core, _ in self._covers.values():        # gradients a fused step left "logically zero" become real zeros before they are read
            core.materialize_grads()
            _distrust_word_moments(core)             # this update writes the moments of every row it covers
        dp = self._dp
        late = []
        if dp is not None and getattr(dp, "late_ranges", None):
            # data parallel: the all-reduce of the LAST backward stage (word embeddings: 94 MB, produced last) is still on the
            # wire.  Everything else is already reduced (the stage hook made this stream wait for the "early" marker only), so
            # the update of those ranges (~78 % of the parameters) runs under that last all-reduce; the late ranges follow after
            # the full wait.
            late = sorted(dp.late_ranges)

        shards = getattr(dp, "shards", None) if dp is not None else None
        grad_scale = self.grad_scale
        if self._clip_value() > 0.0:
            if shards is not None or getattr(dp, "shard_in_engine", False) or (dp is not None and os.environ.get("MB_DP_SHARD_OPT", "0") == "1"):
                raise _lib.MagbertError("max_grad_norm with MB_DP_SHARD_OPT=1: a rank holds only its shard of the reduced gradient, "
                                        "the norm would need a cross-rank sum -- not supported")
            if dp is not None:
                dp.finish()                # the norm needs the WHOLE reduced gradient: no late ranges in such a step
                late = []
            norm, coef = self._clip_coef(L)
            # the product as ONE fp32 multiply: the float the device forms in the single-call step
            grad_scale = float(np.float32(self.grad_scale) * np.float32(coef))
            self._clip_last = (norm, coef)

        def launch(core, group, x, y):
            if shards is not None and core is shards.core and x < shards.hi and y > shards.lo:
                # sharded update (distributed.OptimizerShards): of the layers' GEMM weights only this rank's shard; the rest of
                # [x, y) -- in front of / behind the sharded range -- is replicated as usual
                pieces = [(x, min(y, shards.lo)), (max(x, shards.a), min(y, shards.b)), (max(x, shards.hi), y)]
                for px, py in pieces:
                    if py > px:
                        launch_range(core, group, px, py)
                return
            launch_range(core, group, x, y)

        def launch_range(core, group, x, y):
            if y <= x:
                return
            b1, b2 = group["betas"]
            sh = core.shadow if core.dt == _lib.DT_BF16 else None
            sb = min(max(core.sh_begin, x), y) - x
            se = min(max(core.sh_end, x), y) - x
            _lib.check(L.mb_adamw_step(
                core.params.data_ptr() + 4 * x, core.grads.data_ptr() + 4 * x, core._adam_m.data_ptr() + 4 * x,
                core._adam_v.data_ptr() + 4 * x, (sh.data_ptr() + 2 * x) if sh is not None else None, y - x,
                (y - x) if group["weight_decay"] > 0.0 else 0, sb, se, group["lr"], b1, b2, group["eps"],
                group["weight_decay"], self._t, 1 if group["correct_bias"] else 0, grad_scale,
                1 if self.fused_zero_grad else 0, core.stream()))

        deferred = []                      # (core, group, x, y) pieces that must wait for the last all-reduce
        for item in self._plan:
            group = self.param_groups[item[1]]
            b1, b2 = group["betas"]
            if item[0] == "flat":
                _, _, core, a, b = item
                cur = a
                for lo, n in late:         # split [a, b) around the late ranges (sorted, disjoint, tensor-aligned)
                    hi = lo + n
                    if hi <= cur or lo >= b or core is not dp.core:
                        continue
                    launch(core, group, cur, max(cur, lo))
                    deferred.append((core, group, max(cur, lo), min(b, hi)))
                    cur = min(b, hi)
                launch(core, group, cur, b)
            else:
                p = item[2]
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.MagbertError("AdamW runs on the HIP kernel only: fp32 contiguous ROCm tensors required")
                state = self.state[p]
                if len(state) == 0:
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                g = p.grad.contiguous()
                n = p.numel()
                _lib.check(L.mb_adamw_step(p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(),
                                           state["exp_avg_sq"].data_ptr(), None, n, n if group["weight_decay"] > 0.0 else 0,
                                           0, 0, group["lr"], b1, b2, group["eps"], group["weight_decay"], self._t,
                                           1 if group["correct_bias"] else 0, grad_scale, 0,
                                           torch.cuda.current_stream(p.device).cuda_stream))
        if late:
            dp.finish()                    # this stream now waits for the last all-reduce
            for core, group, x, y in deferred:
                launch(core, group, x, y)
        if shards is not None:
            shards.clear_dead_gradients()  # (before the flag below: the buffer really is all zeros again)
            shards.gather_updated()
        if self.fused_zero_grad:
            self._mark_zero()              # every gradient the update consumed is zero again
        return loss

    # -- checkpoint / resume ---------------------------------------------------------
    def state_dict(self):
        """torch.optim.Optimizer.state_dict() plus what lives outside `self.state`: the step count and, per model, the flat
        Adam moment buffers (tensors on the host, keyed by position among the distinct flat buffers of the plan)."""
        if self._plan is None:
            self._build_plan()
        sd = super().state_dict()
        cores = []
        for item in self._plan:
            if item[0] == "flat" and all(item[2] is not c for c in cores):
                cores.append(item[2])
        # sharded optimizer update under data parallel (MB_DP_SHARD_OPT=1): a rank's moments outside its own slices are stale until
        # gathered.  COLLECTIVE in that mode -- every rank must call state_dict() ("Checkpoints under data parallel").
        for c in cores:
            c.refresh_sharded_state(adam=True)
        sd["magbert"] = {"t": self._t,
                         "flat": [{"exp_avg": c._adam_m.detach().cpu(), "exp_avg_sq": c._adam_v.detach().cpu()} for c in cores]}
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        extra = state_dict.pop("magbert", None)
        super().load_state_dict(state_dict)
        self._plan = None
        self._build_plan()
        if extra is not None:
            self._t = int(extra["t"])
            cores = []
            for item in self._plan:
                if item[0] == "flat" and all(item[2] is not c for c in cores):
                    cores.append(item[2])
            if len(cores) != len(extra["flat"]):
                raise ValueError("optimizer checkpoint holds %d flat buffers, this optimizer has %d" % (len(extra["flat"]), len(cores)))
            for c, st in zip(cores, extra["flat"]):
                c._adam_m.copy_(st["exp_avg"])
                c._adam_v.copy_(st["exp_avg_sq"])
                _distrust_word_moments(c)

    def zero_grad(self, set_to_none=False):
        if self._plan is None:
            self._build_plan()
        done = set()
        for item in self._plan:
            if item[0] == "flat":
                core = item[2]
                if not self.fused_zero_grad and id(core) not in done:
                    core.grads.zero_()
                    core.mark_grads_zero(True)
                    done.add(id(core))
            else:
                p = item[2]
                if p.grad is not None:
                    p.grad.zero_()


def linear_schedule_lambda(current_step, num_warmup_steps, num_training_steps):
    """lr multiplier of transformers 3.0.2 get_linear_schedule_with_warmup (num_warmup_steps may be a float:
    multimodal_driver.py:348 passes warmup_proportion * num_train_optimization_steps)."""
    if current_step < num_warmup_steps:
        return float(current_step) / float(max(1, num_warmup_steps))
    return max(0.0, float(num_training_steps - current_step) / float(max(1, num_training_steps - num_warmup_steps)))


def get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, last_epoch=-1):
    return torch.optim.lr_scheduler.LambdaLR(
        optimizer, lambda s: linear_schedule_lambda(s, num_warmup_steps, num_training_steps), last_epoch)
