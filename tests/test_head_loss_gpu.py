"""The head's two kernels under every objective, through mb_head_forward / mb_head_backward (include/magbert_hip.h), against the fp64
restatement of tests/head_loss_helpers.py computed from the same fp32 inputs.

Tolerance.  The yardstick is the error of the two forms the kernels always had -- MSE at num_labels = 1 and cross entropy at
num_labels = 5, kind 0 -- against fp64, measured here, in this run, through the same entries, on every (H, B) of the sweep and per
output tensor: max |got - want| over the tensor, relative to the largest element of the same expression with every summed term
replaced by its magnitude (head_reference's "scale").  Dividing by max |want| instead measures the draw, not the kernel: the one dbc
entry of nine samples at num_labels = 1 is a sum of mixed signs that came to 1.3e-3 against 0.72 of summed magnitudes in one smooth_l1
case of this sweep, and its fp32 rounding error of 9e-9 then reads as 7e-6.  A new kind gets four times that per tensor: it adds an exp, a log1p or a division by a
summed weight, each a couple of fp32 roundings, and none has a cancellation that its stable form leaves open.  The exact-zero and
exact-limit cases are equalities.  One exception is spelled out where it is asserted: at logit +88 and a target y > 0 the true bce
gradient, -w y sigmoid(-88) / N, is about 6e-39, below fp32's smallest normal number, so "on its limit 0" is asserted as |g| < 2^-126.

MB_HEAD_LOSS_REPORT=<file>: the measured figures per kind and tensor, and the yardstick, are appended there (profiles/head_loss_errors.txt)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_loss_helpers as hl
from bert_multimodal_transformer_amd import _lib, rng

DEV = "cuda:0"
DTS = [(_lib.DT_F32, torch.float32, "fp32"), (_lib.DT_BF16, torch.bfloat16, "bf16")]
HS = (256, 512, 768, 1024)
BS = (1, 3, 4, 5, 9)
NLS = (1, 2, 5)
GUARD = 64              # canary elements behind every buffer
EXTRA_ROWS = 5          # canary rows from B upward: the rest of the last four-sample block and a whole block more
TENSORS = ("pooled", "logits", "loss", "loss_run", "dz", "dWc", "dbc", "dbp")
FIGURES = {}            # (kind label, tensor, dtype name) -> worst error seen in this run


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan_buf(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)


def inputs(H, B, nl, seed=0):
    r = np.random.RandomState(1000 * H + 100 * B + nl + 7919 * seed)
    z = r.randn(B, H).astype(np.float32)
    Wc = (0.05 * r.randn(nl, H)).astype(np.float32)
    bc = (0.3 * r.randn(nl)).astype(np.float32)
    return z, Wc, bc


def targets(kind, B, nl, seed=0):
    r = np.random.RandomState(31 * B + nl + 977 * seed + 5 * hl.CODE[kind])
    kind = hl.resolve(kind, nl)
    if kind == "cross_entropy":
        y = r.randint(0, nl, size=B).astype(np.float32)
        y[0] = nl - 1                        # (the weighted cases give the last class a weight above zero)
        return y
    if kind == "bce":
        y = r.rand(B, nl).astype(np.float32)
        y.reshape(-1)[::3] = np.array([0.0, 1.0, 0.5], np.float32)[np.arange(len(y.reshape(-1)[::3])) % 3]
        return y
    return r.randn(B, nl).astype(np.float32)


def run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, labels, beta=0.0, vec=None, drop=None, loss_scale=1.0, dlogits=None, zero_elems=0):
    """one forward (twice, for loss_run) and one backward inside NaN canaries -> dict of numpy outputs"""
    L = _lib.lib()
    code = hl.CODE[kind]
    rows = B + EXTRA_ROWS
    zd = nan_buf(rows * H + GUARD)
    zd[:B * H] = torch.from_numpy(z).reshape(-1).to(DEV)
    Wd, bd = torch.from_numpy(Wc).to(DEV).contiguous(), torch.from_numpy(bc).to(DEV).contiguous()
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32)).reshape(-1).to(DEV)
    vd = None if vec is None else torch.tensor(vec, dtype=torch.float32, device=DEV)
    pooled, logits = nan_buf(rows * H + GUARD), nan_buf(rows * nl + GUARD)
    lossb = nan_buf(2 + GUARD)
    lossb[:2] = 0.0
    dk = C.byref(drop) if drop is not None else None
    lp, lrp = C.c_void_p(lossb.data_ptr()), C.c_void_p(lossb.data_ptr() + 4)
    fwd = lambda: _lib.check(L.mb_head_forward(_lib.ptr(zd), _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(lab), _lib.ptr(pooled), _lib.ptr(logits),
                                               lp, lrp, B, H, nl, dk, code, float(beta), _lib.ptr(vd), stream()))
    fwd()
    first = lossb[:2].cpu().numpy().copy()
    lossb[0] = 0.0                           # (the caller clears the step's loss; the running sum goes on)
    fwd()
    dz = torch.full((rows * H + GUARD,), float("nan"), dtype=tdt, device=DEV)
    dWc, dbc, dbp = nan_buf(nl * H + GUARD), nan_buf(nl + GUARD), nan_buf(H + GUARD)
    dWc[:nl * H] = 0.0
    dbc[:nl] = 0.0
    dbp[:H] = 0.0
    zp = nan_buf(zero_elems + GUARD) if zero_elems else None
    dl = None if dlogits is None else torch.from_numpy(np.ascontiguousarray(dlogits, dtype=np.float32)).to(DEV)
    _lib.check(L.mb_head_backward(dt, _lib.ptr(dl), _lib.ptr(logits), _lib.ptr(lab), float(loss_scale), _lib.ptr(pooled), _lib.ptr(Wd),
                                  _lib.ptr(dz), _lib.ptr(dWc), _lib.ptr(dbc), _lib.ptr(dbp), _lib.ptr(zp), zero_elems * 4, B, H, nl, dk,
                                  code, float(beta), _lib.ptr(vd), stream()))
    torch.cuda.synchronize()
    # rows from B upward and everything behind the buffers: untouched
    for name, t, n in (("pooled", pooled, B * H), ("logits", logits, B * nl), ("dz", dz, B * H), ("dWc", dWc, nl * H), ("dbc", dbc, nl),
                       ("dbp", dbp, H), ("loss", lossb, 2), ("z", zd, B * H)):
        assert bool(torch.isnan(t[n:].float()).all()), "%s: written behind element %d (H %d B %d nl %d %s)" % (name, n, H, B, nl, kind)
        assert not bool(torch.isnan(t[:n].float()).any()), "%s: NaN inside (H %d B %d nl %d %s)" % (name, H, B, nl, kind)
    if zp is not None:
        assert bool((zp[:zero_elems] == 0).all()) and bool(torch.isnan(zp[zero_elems:]).all()), "zero-fill range"
    second = lossb[:2].cpu().numpy()
    return {"pooled": pooled[:B * H].cpu().numpy().reshape(B, H), "logits": logits[:B * nl].cpu().numpy().reshape(B, nl),
            "loss": np.float32(second[0]), "loss_first": np.float32(first[0]), "loss_run": np.float32(second[1]),
            "dz": dz[:B * H].float().cpu().numpy().reshape(B, H), "dWc": dWc[:nl * H].cpu().numpy().reshape(nl, H),
            "dbc": dbc[:nl].cpu().numpy(), "dbp": dbp[:H].cpu().numpy()}


def errors(got, ref, tensors=TENSORS):
    """max |got - want| per output tensor, relative to the size of what was summed into its elements (head_reference's "scale")"""
    out = {}
    for t in tensors:
        want = np.asarray(2.0 * ref["loss"] if t == "loss_run" else ref[t], np.float64)
        out[t] = float(np.abs(np.asarray(got[t], np.float64) - want).max() / max(ref["scale"][t], 1e-30))
    return out


def measure(H, B, nl, kind, dt, tdt, beta=0.0, vec=None, drop_p=0.0, loss_scale=1.0, seed=0):
    z, Wc, bc = inputs(H, B, nl, seed)
    y = targets(kind, B, nl, seed)
    drop, mask = None, None
    if drop_p > 0:
        key = rng.make_key(17 + seed, 3, rng.SITE_HEAD, drop_p)
        drop = _lib.DropKey(*key)
        mask = rng.keep_mult(B * H, key).reshape(B, H)
    got = run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, y, beta=beta, vec=vec, drop=drop, loss_scale=loss_scale)
    ref = hl.head_reference(z, Wc, bc, y, kind, beta=beta, vec=vec, mask=mask, loss_scale=loss_scale)
    assert got["loss_first"] == got["loss"] or abs(float(got["loss_first"]) - float(got["loss"])) <= 4e-7 * abs(float(got["loss"]))
    return errors(got, ref), got, ref


@pytest.fixture(scope="module")
def yardstick():
    """the parent's two forms, kind 0: per tensor and dz dtype, the worst error over every (H, B) of the sweep"""
    worst = {}
    for dt, tdt, dn in DTS:
        for H in HS:
            for B in BS:
                for nl in (1, 5):
                    err, _, _ = measure(H, B, nl, "default", dt, tdt)
                    for t, e in err.items():
                        worst[(t, dn)] = max(worst.get((t, dn), 0.0), e)
                        FIGURES[("default nl=%d" % nl, t, dn)] = max(FIGURES.get(("default nl=%d" % nl, t, dn), 0.0), e)
    assert all(v > 0 for v in worst.values()), worst
    yield worst
    path = os.environ.get("MB_HEAD_LOSS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# tests/test_head_loss_gpu.py: worst max|got - fp64| / (largest element with every summed term replaced by its magnitude)\n"
                    "# per kind, tensor and dz dtype over H in %s, B in %s, nl in %s, dropout off and at p = 0.1\n" % (HS, BS, NLS))
            f.write("# yardstick = kind 0 (MSE at nl = 1, cross entropy at nl = 5); bound of the new kinds = 4 x yardstick\n")
            for (t, dn), v in sorted(worst.items()):
                f.write("yardstick            %-9s %-4s %.3e   bound %.3e\n" % (t, dn, v, 4 * v))
            for (label, t, dn), v in sorted(FIGURES.items()):
                f.write("%-20s %-9s %-4s %.3e\n" % (label, t, dn, v))


def variants(nl):
    """(label, kind, beta, vec) of the sweep at this width: every legal kind, the vectors absent and present"""
    pw = [3.0] if nl == 1 else ([0.5, 3.0] + [1.0] * (nl - 2))              # pos_weight below and above 1
    out = [("default", "default", 0.0, None), ("mse", "mse", 0.0, None), ("l1", "l1", 0.0, None), ("smooth_l1 beta=1", "smooth_l1", 1.0, None),
           ("smooth_l1 beta=0.3", "smooth_l1", 0.3, None), ("bce", "bce", 0.0, None), ("bce pos_weight", "bce", 0.0, pw)]
    if nl >= 2:
        out += [("cross_entropy", "cross_entropy", 0.0, None),
                ("cross_entropy weight", "cross_entropy", 0.0, [0.0] + [0.75] * (nl - 2) + [1.5])]      # a class of weight 0
    return out


def check(label, err, dn, yardstick):
    for t, e in err.items():
        FIGURES[(label, t, dn)] = max(FIGURES.get((label, t, dn), 0.0), e)
    for t, e in err.items():
        print("%-22s %-9s %-4s err %.3e  yardstick %.3e" % (label, t, dn, e, yardstick[(t, dn)]))
        assert e <= 4.0 * yardstick[(t, dn)], "%s %s %s: error %.3e > 4 x %.3e" % (label, t, dn, e, yardstick[(t, dn)])


@pytest.mark.parametrize("dt,tdt,dn", DTS)
@pytest.mark.parametrize("H", HS)
def test_every_kind_against_fp64(yardstick, H, dt, tdt, dn):
    for B in BS:
        for nl in NLS:
            for label, kind, beta, vec in variants(nl):
                err, got, ref = measure(H, B, nl, kind, dt, tdt, beta=beta, vec=vec, loss_scale=1.0 if B != 5 else 0.5)
                check(label, err, dn, yardstick)


@pytest.mark.parametrize("dt,tdt,dn", DTS)
def test_mse_at_one_label_is_the_default_bit_for_bit(dt, tdt, dn):
    for H, B in ((256, 4), (768, 9), (1024, 5)):
        z, Wc, bc = inputs(H, B, 1)
        y = targets("mse", B, 1)
        a = run_head(H, B, 1, "default", dt, tdt, z, Wc, bc, y[:, 0], loss_scale=0.5)
        b = run_head(H, B, 1, "mse", dt, tdt, z, Wc, bc, y, loss_scale=0.5)
        for t in ("pooled", "logits", "dz") + (("loss", "dWc", "dbc", "dbp") if B <= 4 else ()):       # (one block: no atomic meets another)
            assert np.array_equal(a[t], b[t]), (t, H, B)
        # ... and the unweighted cross entropy is the default at five
        z, Wc, bc = inputs(H, B, 5)
        y = targets("cross_entropy", B, 5)
        a = run_head(H, B, 5, "default", dt, tdt, z, Wc, bc, y)
        b = run_head(H, B, 5, "cross_entropy", dt, tdt, z, Wc, bc, y)
        for t in ("pooled", "logits", "dz") + (("loss", "dWc", "dbc", "dbp") if B <= 4 else ()):
            assert np.array_equal(a[t], b[t]), (t, H, B)


def planted(nl, H=256):
    """zero classifier weights: logit k of every sample is bc[k], exactly"""
    z = np.random.RandomState(3).randn(1, H).astype(np.float32)
    return z, np.zeros((nl, H), np.float32)


def test_kinks_are_exact():
    dt, tdt, _ = DTS[0]
    H = 256
    f = np.float32
    # d == 0: gradient exactly 0 for l1 and smooth_l1 -- B = 5 is two blocks; every sample sits on its target
    bc = np.array([0.75, -1.5], f)
    z = np.random.RandomState(4).randn(5, H).astype(f)
    y = np.tile(bc, (5, 1))
    for kind, beta in (("l1", 0.0), ("smooth_l1", 1.0), ("smooth_l1", 0.0)):
        got = run_head(H, 5, 2, kind, dt, tdt, z, np.zeros((2, H), f), bc, y, beta=beta)
        assert got["loss"] == 0 and not got["dbc"].any() and not got["dWc"].any() and not got["dz"].any() and not got["dbp"].any(), kind
    # one sample, five logits: d = 0, +-beta exactly, and one on each side -- dbc[k] IS the logit gradient of class k
    z, W0 = planted(5)
    for beta in (0.5, 1.0, 2.0):
        bc = np.array([0.25, 1.0, -3.0, 0.5, 8.0], f)
        d = np.array([0.0, beta, -beta, 0.25 * beta, -4.0 * beta], f)
        y = (bc - d).reshape(1, 5)
        assert np.array_equal(bc - y[0], d)                                             # (the planted differences are exact in fp32)
        got = run_head(H, 1, 5, "smooth_l1", dt, tdt, z, W0, bc, y, beta=beta)
        want_g = np.array([0.0, 1.0, -1.0, 0.25, -1.0], f) / f(5)
        assert np.array_equal(got["dbc"], want_g), (beta, got["dbc"], want_g)
        terms = np.array([0.0, 0.5 * beta, 0.5 * beta, 0.5 * 0.0625 * beta, 3.5 * beta], f)      # exact: beta is a power of two
        want_l = f(0)
        for t in terms:
            want_l = f(want_l + t / f(5))
        assert got["loss"] == want_l, (beta, got["loss"], want_l)
        # |d| == beta from the other branch: one ulp more beta puts the same d inside the quadratic piece -- the same value
        inner = run_head(H, 1, 5, "smooth_l1", dt, tdt, z, W0, bc, y, beta=float(np.nextafter(f(beta), f(10))))
        assert np.abs(inner["dbc"].astype(np.float64) - got["dbc"]).max() <= 2 ** -23 and abs(float(inner["loss"]) - float(got["loss"])) <= 2 ** -21 * beta
        l1 = run_head(H, 1, 5, "l1", dt, tdt, z, W0, bc, y)
        assert np.array_equal(l1["dbc"], np.array([0.0, 1.0, -1.0, 1.0, -1.0], f) / f(5))
    # smooth_l1 at beta = 0 gives the bits of l1 (one block: every sum has one order)
    for Hh, B, nl in ((768, 4, 5), (1024, 3, 2), (256, 1, 1)):
        zz, Wc, bcc = inputs(Hh, B, nl)
        yy = targets("l1", B, nl)
        yy[0, 0] = 0.0
        a = run_head(Hh, B, nl, "l1", dt, tdt, zz, Wc, bcc, yy)
        b = run_head(Hh, B, nl, "smooth_l1", dt, tdt, zz, Wc, bcc, yy, beta=0.0)
        for t in TENSORS:
            assert np.array_equal(a[t], b[t]), t


@pytest.mark.parametrize("vec", [None, [0.5, 3.0, 0.5, 3.0]])
def test_bce_limits(yardstick, vec):
    dt, tdt, dn = DTS[0]
    f = np.float32
    H, nl = 256, 4
    z, W0 = planted(nl)
    bc = np.array([1e4, -1e4, 88.0, -88.0], f)
    p = np.ones(nl, f) if vec is None else np.array(vec, f)
    for yv in (0.0, 1.0, 0.5):
        y = np.full((1, nl), yv, f)
        got = run_head(H, 1, nl, "bce", dt, tdt, z, W0, bc, y, vec=vec)
        ref = hl.head_reference(z, W0, bc, y, "bce", vec=vec)
        assert np.isfinite(got["loss"]) and np.array_equal(got["logits"][0], bc)
        assert abs(float(got["loss"]) - ref["loss"]) <= 4 * yardstick[("loss", dn)] * ref["scale"]["loss"], (got["loss"], ref["loss"])
        lw = f(1) + (p - f(1)) * f(yv)
        hi = (f(1) - f(yv)) / f(nl)                      # sigmoid(-x) -> 0: (1 - y) / N
        lo = ((f(1) - f(yv)) - lw) / f(nl)               # sigmoid(-x) -> 1: ((1 - y) - w) / N, which is -pos_weight / N at y = 1
        g = got["dbc"]
        assert g[0] == hi, (yv, g)                       # +1e4
        assert g[1] == lo[1] and g[3] == lo[3], (yv, g, lo)      # -1e4 and -88
        if yv == 0.0:
            assert g[2] == hi
        else:       # the truth, -w y sigmoid(-88) / N ~ 6e-39 (+ (1 - y) / N), is the limit to within fp32's normal range
            assert abs(float(g[2]) - float(hi)) < 2.0 ** -126 or g[2] == hi, (yv, g)
        assert not got["dz"].any()                       # (zero classifier weights)


def test_weighted_cross_entropy_edges(yardstick):
    dt, tdt, dn = DTS[0]
    H, B, nl = 512, 9, 3
    z, Wc, bc = inputs(H, B, nl)
    w = [0.0, 1.5, 0.5]
    y = np.array([0, 1, 0, 2, 1, 0, 2, 2, 1], np.float32)
    got = run_head(H, B, nl, "cross_entropy", dt, tdt, z, Wc, bc, y, vec=w)
    ref = hl.head_reference(z, Wc, bc, y, "cross_entropy", vec=w)
    assert not got["dz"][y == 0].any() and np.abs(got["dz"][y != 0]).max() > 0            # samples of the weight-0 class: exactly 0
    check("cross_entropy weight", errors(got, ref), dn, yardstick)
    y1 = np.full(B, 2, np.float32)                                                       # the whole batch in one class
    got = run_head(H, B, nl, "cross_entropy", dt, tdt, z, Wc, bc, y1, vec=w)
    check("cross_entropy weight", errors(got, hl.head_reference(z, Wc, bc, y1, "cross_entropy", vec=w)), dn, yardstick)


@pytest.mark.parametrize("dt,tdt,dn", DTS)
def test_dropout_replay_and_zero_fill(yardstick, dt, tdt, dn):
    """p = 0.1 with the mask replayed on the host, one case per kind; the zero-fill blocks ride along"""
    H, B = 768, 5
    for nl in (1, 5):
        for label, kind, beta, vec in variants(nl):
            err, got, ref = measure(H, B, nl, kind, dt, tdt, beta=beta, vec=vec, drop_p=0.1, seed=1)
            check(label, err, dn, yardstick)
    z, Wc, bc = inputs(H, B, 5)
    for n in (12, 4 * 1024 * 3 + 20, 4 * 1024 * 600):                                    # a few 16-byte words, several blocks, the block cap
        got = run_head(H, B, 5, "bce", dt, tdt, z, Wc, bc, targets("bce", B, 5), zero_elems=n)
        check("bce", errors(got, hl.head_reference(z, Wc, bc, targets("bce", B, 5), "bce")), dn, yardstick)


def test_given_dlogits_ignore_the_kind(yardstick):
    dt, tdt, dn = DTS[0]
    H, B, nl = 512, 5, 5
    z, Wc, bc = inputs(H, B, nl)
    dl = np.random.RandomState(9).randn(B, nl).astype(np.float32)
    base = None
    for kind in ("default", "l1", "bce", "cross_entropy"):
        got = run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, targets(kind, B, nl), dlogits=dl)
        ref = hl.head_reference(z, Wc, bc, None, kind, dlogits=dl)
        for t, e in errors(got, ref, ("dz", "dWc", "dbc", "dbp")).items():
            assert e <= 4 * yardstick[(t, dn)], (kind, t, e)
        base = base if base is not None else got["dz"]
        assert np.array_equal(got["dz"], base)


def test_refusals():
    L = _lib.lib()
    t = torch.zeros(1024, device=DEV)
    p = _lib.ptr(t)
    assert L.mb_head_forward(p, p, p, p, p, p, p, None, 1, 256, 1, None, 5, 0.0, None, stream()) == 1004       # cross entropy at one label
    assert L.mb_head_forward(p, p, p, p, p, p, p, None, 1, 256, 2, None, 6, 0.0, None, stream()) == 1004       # an unknown kind
    assert L.mb_head_backward(_lib.DT_F32, None, p, p, 1.0, p, p, p, None, None, None, None, 0, 1, 256, 2, None, -1, 0.0, None, stream()) == 1004
    assert L.mb_head_forward(p, p, p, p, p, p, p, None, 1, 320, 1, None, 0, 0.0, None, stream()) == 1001       # H
    torch.cuda.synchronize()
