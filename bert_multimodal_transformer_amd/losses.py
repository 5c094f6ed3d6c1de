"""The objective of the fused classification head (csrc/head.hip, include/magbert_hip.h: mb_*_set_head_loss).

A head loss is a kind plus at most one scalar (smooth_l1's beta) and one vector of num_labels floats (bce's pos_weight, the cross
entropy's class weights), with the semantics of torch.nn.functional's function of the same name under mean reduction.  `default` is
what the reference's classes hard-wire: MSE at num_labels == 1, cross entropy on class indices otherwise.  Everything here is host
code with no engine behind it: what set_loss / from_pretrained accept, what labels a kind takes, and the torch function the
autograd route applies, so that a model's two routes cannot disagree.

Options (the `_ex` entries of include/magbert_hip.h).  cross_entropy takes label_smoothing (0 <= eps < 1), ignore_index (any integer: a
label equal to it is left out of the loss, the gradient and the normaliser, even where it names a real class) and focal_gamma (0, or
finite and >= 1; not together with label_smoothing); bce takes focal_gamma (the sigmoid focal loss, pos_weight as its alpha).  The
cross entropy is normalised by W, the summed class weights -- or the count -- of the kept samples.  ONE deliberate departure from torch:
at W == 0 (every sample ignored, or every kept sample in a class of weight 0) the loss and its gradients are 0, where torch returns
NaN: a NaN must never reach the optimizer's moments.  Not built: 0 < gamma < 1, an alpha other than weight / pos_weight, ignore_index
for bce or the default kind, per-sample weights, reductions other than mean, a normaliser taken across data-parallel ranks."""
import math
import operator

import torch

LOSS_DEFAULT, LOSS_MSE, LOSS_L1, LOSS_SMOOTH_L1, LOSS_BCE, LOSS_CROSS_ENTROPY = range(6)
LOSSES = {"default": LOSS_DEFAULT, "mse": LOSS_MSE, "l1": LOSS_L1, "smooth_l1": LOSS_SMOOTH_L1, "bce": LOSS_BCE,
          "cross_entropy": LOSS_CROSS_ENTROPY}
PER_ELEMENT = ("mse", "l1", "smooth_l1", "bce")          # labels [B, num_labels]; the others take [B]
_KINDS = ", ".join(LOSSES)


class HeadLoss(object):
    """what model.loss returns: name, beta (smooth_l1 only, else None), pos_weight (bce) / weight (cross_entropy) as tuples or None,
    and the options label_smoothing, ignore_index, focal_gamma (None = not set; a smoothing or gamma of 0 is stored as None)"""

    def __init__(self, name="default", beta=None, pos_weight=None, weight=None, label_smoothing=None, ignore_index=None, focal_gamma=None):
        self.name, self.beta, self.pos_weight, self.weight = name, beta, pos_weight, weight
        self.label_smoothing, self.ignore_index, self.focal_gamma = label_smoothing, ignore_index, focal_gamma

    def _key(self):
        return (self.name, self.beta, self.pos_weight, self.weight, self.label_smoothing, self.ignore_index, self.focal_gamma)

    @property
    def code(self):
        return LOSSES[self.name]

    @property
    def vector(self):
        return self.pos_weight if self.name == "bce" else self.weight if self.name == "cross_entropy" else None

    @property
    def per_element(self):
        return self.name in PER_ELEMENT

    def __eq__(self, other):
        return isinstance(other, HeadLoss) and self._key() == other._key()

    def __repr__(self):
        extra = [("beta", self.beta), ("pos_weight", self.pos_weight), ("weight", self.weight), ("label_smoothing", self.label_smoothing),
                 ("ignore_index", self.ignore_index), ("focal_gamma", self.focal_gamma)]
        return "HeadLoss(%s)" % ", ".join([repr(self.name)] + ["%s=%r" % kv for kv in extra if kv[1] is not None])


def _vector(values, what, num_labels):
    if torch.is_tensor(values):
        values = values.detach().cpu().reshape(-1).tolist()
    vals = tuple(float(v) for v in values)
    if len(vals) != num_labels:
        raise ValueError("%s: expected %d values (num_labels), got %d" % (what, num_labels, len(vals)))
    if any(not math.isfinite(v) or v < 0 for v in vals) or not any(v > 0 for v in vals):
        raise ValueError("%s must be finite, non-negative and not all zero, got %s" % (what, list(vals)))
    return vals


def make_loss(name, num_labels, beta=None, pos_weight=None, weight=None, label_smoothing=None, ignore_index=None, focal_gamma=None):
    """the checked HeadLoss of set_loss(name, beta=, pos_weight=, weight=, label_smoothing=, ignore_index=, focal_gamma=) on a model of
    num_labels outputs; ValueError otherwise"""
    if not isinstance(name, str) or name not in LOSSES:
        raise ValueError("loss=%r: the head losses built are %s" % (name, _KINDS))
    takes = {"smooth_l1": ("beta",), "bce": ("pos_weight", "focal_gamma"),
             "cross_entropy": ("weight", "label_smoothing", "ignore_index", "focal_gamma")}.get(name, ())
    for arg, val in (("beta", beta), ("pos_weight", pos_weight), ("weight", weight), ("label_smoothing", label_smoothing),
                     ("ignore_index", ignore_index), ("focal_gamma", focal_gamma)):
        if val is not None and arg not in takes:
            raise ValueError("loss=%r takes no %s (the head losses built are %s; beta belongs to smooth_l1, pos_weight to bce, "
                             "weight, label_smoothing and ignore_index to cross_entropy, focal_gamma to cross_entropy and bce)"
                             % (name, arg, _KINDS))
    if name == "cross_entropy" and num_labels < 2:
        raise ValueError("loss='cross_entropy' needs num_labels >= 2 (of %s, a model of one output takes mse, l1, smooth_l1 or bce)" % _KINDS)
    if name == "smooth_l1":
        beta = 1.0 if beta is None else float(beta)
        if not math.isfinite(beta) or beta < 0:
            raise ValueError("smooth_l1: beta must be finite and >= 0, got %r" % beta)
    if pos_weight is not None:
        pos_weight = _vector(pos_weight, "pos_weight", num_labels)
    if weight is not None:
        weight = _vector(weight, "weight", num_labels)
    if label_smoothing is not None:
        label_smoothing = float(label_smoothing)
        if not 0.0 <= label_smoothing < 1.0:                 # (NaN fails both comparisons)
            raise ValueError("label_smoothing must lie in [0, 1), got %r (the head losses built are %s)" % (label_smoothing, _KINDS))
    if focal_gamma is not None:
        focal_gamma = float(focal_gamma)
        if not (focal_gamma == 0.0 or (math.isfinite(focal_gamma) and focal_gamma >= 1.0)):
            raise ValueError("focal_gamma must be 0, or finite and >= 1 (0 < gamma < 1 is not built), got %r (the head losses built "
                             "are %s)" % (focal_gamma, _KINDS))
    if label_smoothing and focal_gamma:
        raise ValueError("label_smoothing and focal_gamma cannot be combined (the head losses built are %s)" % _KINDS)
    if ignore_index is not None:
        try:
            if isinstance(ignore_index, bool):
                raise TypeError
            ignore_index = operator.index(ignore_index)
        except TypeError:
            raise ValueError("ignore_index must be an integer or None, got %r (the head losses built are %s)" % (ignore_index, _KINDS))
        if not -2 ** 24 <= ignore_index <= 2 ** 24:          # class indices travel as fp32
            raise ValueError("ignore_index %d does not survive fp32 labels (the head losses built are %s)" % (ignore_index, _KINDS))
    return HeadLoss(name, beta, pos_weight, weight, label_smoothing or None, ignore_index, focal_gamma or None)


def check_labels(loss, labels, B, num_labels):
    """labels (a tensor, flattened or not) against what the kind reads; ValueError on a wrong count, a bce target outside [0, 1], a
    class index torch's cross_entropy would reject or treat specially (a label equal to the configured ignore_index passes), or a
    batch whose every label is ignored"""
    n = labels.numel()
    if loss.per_element:
        if n != B * num_labels:
            raise ValueError("labels: loss %r reads one target per logit, expected %d x %d = %d values, got %d"
                             % (loss.name, B, num_labels, B * num_labels, n))
        if loss.name == "bce":
            lf = labels.detach().float()
            if bool(((lf < 0) | (lf > 1) | (lf != lf)).any()):
                raise ValueError("labels of the fused bce must lie in [0, 1]")
        return
    if n != B:
        raise ValueError("labels: expected %d values for a batch of %d, got %d" % (B, B, n))
    if num_labels > 1:
        # fused cross entropy (head.hip): class indices travel as fp32; what torch's CrossEntropyLoss would reject or treat
        # specially must not silently become class 0 (-100 passes only as the ignore_index that set_loss was given)
        lf = labels.detach().float().reshape(-1)
        bad = (lf != lf.round()) | (lf < 0) | (lf >= num_labels)
        ignore = loss.ignore_index if loss.name == "cross_entropy" else None
        if ignore is None:
            if bool(bad.any()):
                raise ValueError("labels of the fused cross entropy must be class indices in [0, %d) (no ignore_index is set)" % num_labels)
            return
        ignored = lf == float(ignore)
        nbad, nkept = (int(v) for v in torch.stack([(bad & ~ignored).sum(), (~ignored).sum()]).tolist())
        if nbad:
            raise ValueError("labels of the fused cross entropy must be class indices in [0, %d) or the ignore_index %d" % (num_labels, ignore))
        if nkept == 0:
            raise ValueError("labels: every label of the batch equals the ignore_index %d: nothing to train on" % ignore)


def _focal_cross_entropy(loss, x, y, vec):
    keep = torch.ones_like(y, dtype=torch.bool) if loss.ignore_index is None else y != loss.ignore_index
    ys = torch.where(keep, y, torch.zeros_like(y))
    onehot = torch.nn.functional.one_hot(ys, x.shape[1]).to(x.dtype)
    logp = (torch.log_softmax(x, dim=1) * onehot).sum(dim=1)
    one_minus_p = (torch.softmax(x, dim=1) * (1.0 - onehot)).sum(dim=1)          # from the non-target classes, not 1 - p
    w = (torch.ones_like(logp) if vec is None else vec[ys]) * keep.to(x.dtype)
    W = w.sum()
    if float(W) == 0.0:
        return x.sum() * 0
    return (w * one_minus_p.pow(loss.focal_gamma) * -logp).sum() / W


def torch_loss(loss, logits, labels, num_labels):
    """the same objective by torch.nn.functional, on logits [B, num_labels]: what forward(labels=...) returns.  At W == 0 (module
    docstring) it returns logits.sum() * 0: a zero with zero gradients, where torch's cross_entropy gives NaN."""
    F = torch.nn.functional
    labels = labels.to(logits.device)
    vec = None if loss.vector is None else torch.tensor(loss.vector, dtype=logits.dtype, device=logits.device)
    if loss.name == "default":
        if num_labels == 1:
            return F.mse_loss(logits.view(-1), labels.float().view(-1))
        return F.cross_entropy(logits.view(-1, num_labels), labels.view(-1))
    if loss.name == "cross_entropy":
        x, y = logits.view(-1, num_labels), labels.view(-1).long()
        if loss.focal_gamma:
            return _focal_cross_entropy(loss, x, y, vec)
        if loss.ignore_index is None and not (loss.weight and 0.0 in loss.weight):
            return F.cross_entropy(x, y, weight=vec, label_smoothing=loss.label_smoothing or 0.0)
        ignore = -100 if loss.ignore_index is None else loss.ignore_index
        keep = y != ignore
        W = keep.sum() if vec is None else (vec[torch.where(keep, y, torch.zeros_like(y))] * keep.to(vec.dtype)).sum()
        if float(W) == 0.0:
            return x.sum() * 0
        return F.cross_entropy(x, y, weight=vec, ignore_index=ignore, label_smoothing=loss.label_smoothing or 0.0)
    x, y = logits.reshape(-1, num_labels), labels.to(logits.dtype).reshape(-1, num_labels)
    if loss.name == "mse":
        return F.mse_loss(x, y)
    if loss.name == "l1":
        return F.l1_loss(x, y)
    if loss.name == "smooth_l1":
        return F.smooth_l1_loss(x, y, beta=loss.beta)
    if loss.focal_gamma:                # sigmoid focal loss: (1 - p_t)^gamma times today's term, pos_weight included
        one_minus_pt = y * torch.sigmoid(-x) + (1.0 - y) * torch.sigmoid(x)
        return (one_minus_pt.pow(loss.focal_gamma) * F.binary_cross_entropy_with_logits(x, y, pos_weight=vec, reduction="none")).mean()
    return F.binary_cross_entropy_with_logits(x, y, pos_weight=vec)
