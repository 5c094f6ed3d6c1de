"""The objective of the fused classification head (csrc/head.hip, include/magbert_hip.h: mb_*_set_head_loss).

A head loss is a kind plus at most one scalar (smooth_l1's beta) and one vector of num_labels floats (bce's pos_weight, the cross
entropy's class weights), with the semantics of torch.nn.functional's function of the same name under mean reduction.  `default` is
what the reference's classes hard-wire: MSE at num_labels == 1, cross entropy on class indices otherwise.  Everything here is host
code with no engine behind it: what set_loss / from_pretrained accept, what labels a kind takes, and the torch function the
autograd route applies, so that a model's two routes cannot disagree."""
import math

import torch

LOSS_DEFAULT, LOSS_MSE, LOSS_L1, LOSS_SMOOTH_L1, LOSS_BCE, LOSS_CROSS_ENTROPY = range(6)
LOSSES = {"default": LOSS_DEFAULT, "mse": LOSS_MSE, "l1": LOSS_L1, "smooth_l1": LOSS_SMOOTH_L1, "bce": LOSS_BCE,
          "cross_entropy": LOSS_CROSS_ENTROPY}
PER_ELEMENT = ("mse", "l1", "smooth_l1", "bce")          # labels [B, num_labels]; the others take [B]
_KINDS = ", ".join(LOSSES)


class HeadLoss(object):
    """what model.loss returns: name, beta (smooth_l1 only, else None), pos_weight (bce) / weight (cross_entropy) as tuples or None"""

    def __init__(self, name="default", beta=None, pos_weight=None, weight=None):
        self.name, self.beta, self.pos_weight, self.weight = name, beta, pos_weight, weight

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
        return isinstance(other, HeadLoss) and (self.name, self.beta, self.pos_weight, self.weight) == \
            (other.name, other.beta, other.pos_weight, other.weight)

    def __repr__(self):
        extra = [("beta", self.beta), ("pos_weight", self.pos_weight), ("weight", self.weight)]
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


def make_loss(name, num_labels, beta=None, pos_weight=None, weight=None):
    """the checked HeadLoss of set_loss(name, beta=, pos_weight=, weight=) on a model of num_labels outputs; ValueError otherwise"""
    if not isinstance(name, str) or name not in LOSSES:
        raise ValueError("loss=%r: the head losses built are %s" % (name, _KINDS))
    takes = {"smooth_l1": ("beta",), "bce": ("pos_weight",), "cross_entropy": ("weight",)}.get(name, ())
    for arg, val in (("beta", beta), ("pos_weight", pos_weight), ("weight", weight)):
        if val is not None and arg not in takes:
            raise ValueError("loss=%r takes no %s (the head losses built are %s; beta belongs to smooth_l1, pos_weight to bce, "
                             "weight to cross_entropy)" % (name, arg, _KINDS))
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
    return HeadLoss(name, beta, pos_weight, weight)


def check_labels(loss, labels, B, num_labels):
    """labels (a tensor, flattened or not) against what the kind reads; ValueError on a wrong count, a bce target outside [0, 1], or a
    class index torch's cross_entropy would reject or treat specially"""
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
        # specially must not silently become class 0 (ignore_index = -100 is not built)
        lf = labels.detach().float().reshape(-1)
        if bool(((lf != lf.round()) | (lf < 0) | (lf >= num_labels)).any()):
            raise ValueError("labels of the fused cross entropy must be class indices in [0, %d) (ignore_index is not supported)" % num_labels)


def torch_loss(loss, logits, labels, num_labels):
    """the same objective by torch.nn.functional, on logits [B, num_labels]: what forward(labels=...) returns"""
    F = torch.nn.functional
    labels = labels.to(logits.device)
    vec = None if loss.vector is None else torch.tensor(loss.vector, dtype=logits.dtype, device=logits.device)
    if loss.name == "default":
        if num_labels == 1:
            return F.mse_loss(logits.view(-1), labels.float().view(-1))
        return F.cross_entropy(logits.view(-1, num_labels), labels.view(-1))
    if loss.name == "cross_entropy":
        return F.cross_entropy(logits.view(-1, num_labels), labels.view(-1).long(), weight=vec)
    x, y = logits.reshape(-1, num_labels), labels.to(logits.dtype).reshape(-1, num_labels)
    if loss.name == "mse":
        return F.mse_loss(x, y)
    if loss.name == "l1":
        return F.l1_loss(x, y)
    if loss.name == "smooth_l1":
        return F.smooth_l1_loss(x, y, beta=loss.beta)
    return F.binary_cross_entropy_with_logits(x, y, pos_weight=vec)
