"""fp64 restatement of the fused head and its objectives (csrc/head.hip; the table of include/magbert_hip.h: mb_head_forward),
written from the formulas -- no torch loss is called here.  tests/test_head_loss_cpu.py pins it against torch.nn.functional;
the GPU tests take it as their expectation."""
import numpy as np

KINDS = ("default", "mse", "l1", "smooth_l1", "bce", "cross_entropy")
CODE = {k: i for i, k in enumerate(KINDS)}
PER_ELEMENT = ("mse", "l1", "smooth_l1", "bce")


def resolve(kind, nl):
    """the kind the default stands for at this width"""
    if kind == "default":
        return "mse" if nl == 1 else "cross_entropy"
    return kind


def legal_kinds(nl):
    return [k for k in KINDS if not (k == "cross_entropy" and nl < 2)]


def loss_and_grad(kind, logits, labels, beta=None, vec=None):
    """logits [B, nl]; labels [B, nl] (per-element kinds) or [B] class indices / targets -> (loss, d loss / d logits [B, nl]), fp64.
    beta: smooth_l1's; vec: bce's pos_weight or the cross entropy's class weights ([nl] or None).  Mean reduction."""
    x = np.asarray(logits, np.float64)
    B, nl = x.shape
    kind = resolve(kind, nl)
    if kind == "cross_entropy":
        y = np.asarray(labels).reshape(B).astype(np.int64)
        w = np.ones(nl) if vec is None else np.asarray(vec, np.float64)
        mx = x.max(axis=1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
        nll = lse - x[np.arange(B), y]
        wy = w[y]
        den = wy.sum()
        soft = np.exp(x - lse[:, None])
        onehot = np.zeros_like(x)
        onehot[np.arange(B), y] = 1.0
        return float((wy * nll).sum() / den), wy[:, None] * (soft - onehot) / den
    y = np.asarray(labels, np.float64).reshape(B, nl)
    d = x - y
    n = float(B * nl)
    sign = (d > 0).astype(np.float64) - (d < 0).astype(np.float64)
    if kind == "mse":
        return float((d * d).sum() / n), 2.0 * d / n
    if kind == "l1":
        return float(np.abs(d).sum() / n), sign / n
    if kind == "smooth_l1":
        b = 1.0 if beta is None else float(beta)
        ad = np.abs(d)
        inner = ad < b                               # beta == 0: never, the expressions of l1
        with np.errstate(divide="ignore", invalid="ignore"):
            quad = np.where(inner, 0.5 * d * d / b, 0.0) if b > 0 else np.zeros_like(d)
            gquad = np.where(inner, d / b, 0.0) if b > 0 else np.zeros_like(d)
        val = np.where(inner, quad, ad - 0.5 * b)
        return float(val.sum() / n), np.where(inner, gquad, sign) / n
    assert kind == "bce", kind
    p = np.ones(nl) if vec is None else np.asarray(vec, np.float64)
    lw = 1.0 + (p[None, :] - 1.0) * y
    e = np.exp(-np.abs(x))
    softplus_neg = np.maximum(-x, 0.0) + np.log1p(e)          # log(1 + exp(-x)), stable in both tails
    sig_neg = np.where(x >= 0, e, 1.0) / (1.0 + e)            # sigmoid(-x)
    val = (1.0 - y) * x + lw * softplus_neg
    return float(val.sum() / n), ((1.0 - y) - lw * sig_neg) / n


def loss_magnitude(kind, logits, labels, beta=None, vec=None):
    """the loss with every term of its sum replaced by its magnitude: what a rounding error of that sum is relative to.  The regression
    kinds sum non-negative terms (it is the loss itself); bce's (1 - y) x and the cross entropy's lse - x_y can cancel."""
    x = np.asarray(logits, np.float64)
    B, nl = x.shape
    kind = resolve(kind, nl)
    if kind == "cross_entropy":
        y = np.asarray(labels).reshape(B).astype(np.int64)
        w = np.ones(nl) if vec is None else np.asarray(vec, np.float64)
        mx = x.max(axis=1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
        return float((w[y] * (np.abs(lse) + np.abs(x[np.arange(B), y]))).sum() / w[y].sum())
    if kind == "bce":
        y = np.asarray(labels, np.float64).reshape(B, nl)
        p = np.ones(nl) if vec is None else np.asarray(vec, np.float64)
        lw = 1.0 + (p[None, :] - 1.0) * y
        return float((np.abs((1.0 - y) * x) + lw * (np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x))))).sum() / (B * nl))
    return loss_and_grad(kind, x, labels, beta=beta, vec=vec)[0]


def head_reference(z, Wc, bc, labels, kind, beta=None, vec=None, mask=None, loss_scale=1.0, dlogits=None):
    """The head in fp64 from fp32 inputs: z [B, H] pooler pre-activations, Wc [nl, H], bc [nl], mask [B, H] dropout multipliers or
    None.  -> dict(pooled, logits, loss, dlogits, dz, dWc, dbc, dbp); the gradients are those of loss_scale * loss (or of `dlogits`).
    "scale" holds, per output, the largest element of the same expression with every term of every sum replaced by its magnitude:
    a sum that cancels (nine logit gradients of mixed sign adding up to 1e-3 of their size in one dbc entry) is then judged by what
    was summed, as floating-point error bounds are stated, not by what happened to be left over."""
    z, Wc, bc = (np.asarray(a, np.float64) for a in (z, Wc, bc))
    m = np.ones_like(z) if mask is None else np.asarray(mask, np.float64)
    pooled = np.tanh(z)
    pd = pooled * m
    logits = pd @ Wc.T + bc
    out = {"pooled": pooled, "logits": logits}
    if dlogits is None:
        loss, g = loss_and_grad(kind, logits, labels, beta=beta, vec=vec)
        out["loss"] = loss
        dl = g * loss_scale
    else:
        dl = np.asarray(dlogits, np.float64)
    out["dlogits"] = dl
    out["dWc"] = dl.T @ pd
    out["dbc"] = dl.sum(axis=0)
    out["dz"] = (dl @ Wc) * m * (1.0 - pooled * pooled)
    out["dbp"] = out["dz"].sum(axis=0)
    adl, apd = np.abs(dl), np.abs(pd)
    adz = (adl @ np.abs(Wc)) * m * (1.0 - pooled * pooled)
    out["scale"] = {"pooled": float(np.abs(pooled).max()), "logits": float((apd @ np.abs(Wc).T + np.abs(bc)).max()),
                    "dz": float(adz.max()), "dWc": float((adl.T @ apd).max()), "dbc": float(adl.sum(axis=0).max()),
                    "dbp": float(adz.sum(axis=0).max())}
    if dlogits is None:
        out["scale"]["loss"] = loss_magnitude(kind, logits, labels, beta=beta, vec=vec)
        out["scale"]["loss_run"] = 2.0 * out["scale"]["loss"]
    return out
