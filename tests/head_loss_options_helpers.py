"""fp64 restatement of the head's objectives under their options -- label smoothing, ignore_index and the focal exponent (csrc/head.hip;
mb_head_loss of include/magbert_hip.h) -- written from the formulas, no torch loss is called here.  tests/test_head_loss_options_cpu.py
pins it against torch.nn.functional with autograd; the GPU tests take it as their expectation.  Without options it IS
head_loss_helpers.loss_and_grad.

cross entropy, q = softmax(x_b), kept = (y_b != ignore), w = 1 without weights, W = sum over kept b of w[y_b]:
    smoothing e:  [ (1-e) sum_kept w[y_b] (-log q_by) + (e/C) sum_kept sum_k w_k (-log q_bk) ] / W
    focal g:      sum_kept w[y_b] (1 - p)^g (-log p) / W,  p = q_by
    W == 0:       loss 0, gradient 0 (torch: NaN)
bce, focal g:     mean of (1 - p_t)^g l,  l = bce's term with pos_weight,  1 - p_t = y sigmoid(-x) + (1 - y) sigmoid(x)"""
import numpy as np

import head_loss_helpers as hl


def _pow(u, g):
    """u^g for u >= 0 with u^0 == 1 everywhere"""
    u = np.asarray(u, np.float64)
    if g == 0:
        return np.ones_like(u)
    return np.where(u > 0, np.power(np.maximum(u, 1e-300), g), 0.0)


def _ce_parts(x, labels, vec, ignore):
    B, nl = x.shape
    y = np.asarray(labels).reshape(B).astype(np.int64)
    keep = np.ones(B, bool) if ignore is None else y != int(ignore)      # the ignore test comes before the weight lookup
    ys = np.where(keep, y, 0)
    w = np.ones(nl) if vec is None else np.asarray(vec, np.float64)
    mx = x.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
    q = np.exp(x - lse[:, None])
    onehot = np.zeros_like(x)
    onehot[np.arange(B), ys] = 1.0
    wy = np.where(keep, w[ys], 0.0)
    omp = (q * (1.0 - onehot)).sum(axis=1)                               # 1 - p from the non-target classes
    nlp = np.where(omp < 0.5, -np.log1p(-np.minimum(omp, 0.5)), lse - x[np.arange(B), ys])
    return keep, ys, w, lse, q, onehot, wy, omp, nlp


def loss_and_grad(kind, logits, labels, beta=None, vec=None, smoothing=0.0, ignore=None, gamma=0.0):
    """as head_loss_helpers.loss_and_grad, with the options -> (loss, d loss / d logits [B, nl]), fp64"""
    x = np.asarray(logits, np.float64)
    B, nl = x.shape
    kind = hl.resolve(kind, nl)
    if not smoothing and ignore is None and not gamma:
        return hl.loss_and_grad(kind, x, labels, beta=beta, vec=vec)
    assert not (smoothing and gamma)
    if kind == "cross_entropy":
        keep, ys, w, lse, q, onehot, wy, omp, nlp = _ce_parts(x, labels, vec, ignore)
        W = wy.sum()
        if W == 0:
            return 0.0, np.zeros_like(x)
        if gamma:
            p = q[np.arange(B), ys]
            loss = (wy * _pow(omp, gamma) * nlp).sum() / W
            fac = _pow(omp, gamma) + gamma * p * _pow(omp, gamma - 1.0) * nlp
            dq = np.where(onehot > 0, -omp[:, None], q)                  # q_k - [k == y], the target's entry as -(1 - p)
            return float(loss), (wy * fac)[:, None] * dq / W
        e = float(smoothing)
        nll = lse - x[np.arange(B), ys]
        allk = (w[None, :] * (lse[:, None] - x)).sum(axis=1)
        k = keep.astype(np.float64)
        loss = ((1.0 - e) * (wy * nll).sum() + e / nl * (k * allk).sum()) / W
        g = ((1.0 - e) * wy[:, None] * (q - onehot) + e / nl * k[:, None] * (q * w.sum() - w[None, :])) / W
        return float(loss), g
    assert kind == "bce" and gamma and not smoothing and ignore is None, (kind, smoothing, ignore, gamma)
    y = np.asarray(labels, np.float64).reshape(B, nl)
    n = float(B * nl)
    l, dl = hl.loss_and_grad("bce", x, y, vec=vec)                       # mean and its gradient: term = n * contribution
    p = np.ones(nl) if vec is None else np.asarray(vec, np.float64)
    lw = 1.0 + (p[None, :] - 1.0) * y
    ex = np.exp(-np.abs(x))
    sn, sp = np.where(x >= 0, ex, 1.0) / (1.0 + ex), np.where(x >= 0, 1.0, ex) / (1.0 + ex)
    term = (1.0 - y) * x + lw * (np.maximum(-x, 0.0) + np.log1p(ex))
    dterm = dl * n
    m = y * sn + (1.0 - y) * sp
    dm = sp * sn * (1.0 - 2.0 * y)
    val = _pow(m, gamma) * term
    return float(val.sum() / n), (gamma * _pow(m, gamma - 1.0) * dm * term + _pow(m, gamma) * dterm) / n


def loss_magnitude(kind, logits, labels, beta=None, vec=None, smoothing=0.0, ignore=None, gamma=0.0):
    """the loss with every term of its sums replaced by its magnitude (head_loss_helpers.loss_magnitude under the options)"""
    x = np.asarray(logits, np.float64)
    B, nl = x.shape
    kind = hl.resolve(kind, nl)
    if not smoothing and ignore is None and not gamma:
        return hl.loss_magnitude(kind, x, labels, beta=beta, vec=vec)
    if kind == "cross_entropy":
        keep, ys, w, lse, q, onehot, wy, omp, nlp = _ce_parts(x, labels, vec, ignore)
        W = wy.sum()
        if W == 0:
            return 0.0
        mag = np.abs(lse) + np.abs(x[np.arange(B), ys])
        if gamma:
            return float((wy * _pow(omp, gamma) * mag).sum() / W)
        e = float(smoothing)
        allk = (w[None, :] * (np.abs(lse)[:, None] + np.abs(x))).sum(axis=1)
        return float(((1.0 - e) * (wy * mag).sum() + e / nl * (keep * allk).sum()) / W)
    y = np.asarray(labels, np.float64).reshape(B, nl)
    p = np.ones(nl) if vec is None else np.asarray(vec, np.float64)
    lw = 1.0 + (p[None, :] - 1.0) * y
    ex = np.exp(-np.abs(x))
    sn, sp = np.where(x >= 0, ex, 1.0) / (1.0 + ex), np.where(x >= 0, 1.0, ex) / (1.0 + ex)
    m = y * sn + (1.0 - y) * sp
    return float((_pow(m, gamma) * (np.abs((1.0 - y) * x) + lw * (np.maximum(-x, 0.0) + np.log1p(ex)))).sum() / (B * nl))


def head_reference(z, Wc, bc, labels, kind, beta=None, vec=None, mask=None, loss_scale=1.0, smoothing=0.0, ignore=None, gamma=0.0):
    """head_loss_helpers.head_reference under the options: the same dict (pooled, logits, loss, dlogits, dz, dWc, dbc, dbp, scale)"""
    first = hl.head_reference(z, Wc, bc, None, kind, mask=mask, dlogits=np.zeros((np.asarray(z).shape[0], np.asarray(Wc).shape[0])))
    loss, g = loss_and_grad(kind, first["logits"], labels, beta=beta, vec=vec, smoothing=smoothing, ignore=ignore, gamma=gamma)
    out = hl.head_reference(z, Wc, bc, None, kind, mask=mask, dlogits=g * loss_scale)
    out["loss"] = loss
    out["scale"]["loss"] = loss_magnitude(kind, out["logits"], labels, beta=beta, vec=vec, smoothing=smoothing, ignore=ignore, gamma=gamma)
    out["scale"]["loss_run"] = 2.0 * out["scale"]["loss"]
    return out
