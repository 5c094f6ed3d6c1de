"""The head's two kernels under the loss options -- label smoothing, ignore_index, the focal exponent -- through mb_head_forward_ex /
mb_head_backward_ex (include/magbert_hip.h), against the fp64 restatement of tests/head_loss_options_helpers.py computed from the same
fp32 inputs.  NaN canaries, guard rows and both dz dtypes as tests/test_head_loss_gpu.py::run_head has them.

Tolerance: the method of tests/test_head_loss_gpu.py.  The yardstick is the error of kind 0 -- MSE at num_labels = 1 and cross entropy at
num_labels = 5, the forms the kernels always had -- against fp64, measured in this run through the same `_ex` entries (a neutral
mb_head_loss) on every (H, B) of the sweep and per output tensor: max |got - want| relative to the largest element of the same
expression with every summed term replaced by its magnitude.  An option gets four times that per tensor, the factor the existing file
argues for a new kind: smoothing adds one weighted sum over the classes, the focal factor an exp, a log1p and a pow, the normaliser a
division by a summed weight -- each a few fp32 roundings, and none leaves a cancellation open (1 - p is summed from the non-target
exponentials, log p taken by log1p where p > 0.5).  The yardstick is never the code under test.  Exact zeros and bit equalities are
asserted as equalities; sub-normal limits as the existing file treats them (|g - limit| < 2^-126).

Shapes: H = 256, 768, 1024 (one, three, four column chunks); B = 1, 3, 4, 5, 9 (a partial block, a whole block, one sample past it);
B = 65 and 130 at H = 256 (65: the first batch that gives the lane-strided normaliser a second trip); C = 2, 5; bce at 1 and 3 labels.

MB_HEAD_LOSS_REPORT=<file>: the measured figures per case and tensor, and the yardstick, are appended (profiles/head_loss_options_errors.txt)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_loss_helpers as hl
import head_loss_options_helpers as ho
from bert_multimodal_transformer_amd import _lib

DEV = "cuda:0"
DTS = [(_lib.DT_F32, torch.float32, "fp32"), (_lib.DT_BF16, torch.bfloat16, "bf16")]
HS = (256, 768, 1024)
BS = (1, 3, 4, 5, 9)
GUARD = 64              # canary elements behind every buffer
EXTRA_ROWS = 5          # canary rows from B upward: the rest of the last four-sample block and a whole block more
TENSORS = ("pooled", "logits", "loss", "loss_run", "dz", "dWc", "dbc", "dbp")
GRADS = ("dz", "dWc", "dbc", "dbp")
FIGURES = {}            # (case label, tensor, dtype name) -> worst error seen in this run
IGN = -100


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan_buf(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)


def inputs(H, B, nl, seed=0):
    r = np.random.RandomState(1000 * H + 100 * B + nl + 7919 * seed)
    return r.randn(B, H).astype(np.float32), (0.05 * r.randn(nl, H)).astype(np.float32), (0.3 * r.randn(nl)).astype(np.float32)


def targets(kind, B, nl, seed=0):
    r = np.random.RandomState(31 * B + nl + 977 * seed + 5 * hl.CODE[kind])
    kind = hl.resolve(kind, nl)
    if kind == "cross_entropy":
        y = r.randint(0, nl, size=B).astype(np.float32)
        y[-1] = nl - 1
        return y
    if kind == "bce":
        y = (r.rand(B, nl) < 0.5).astype(np.float32)                    # hard targets, and a few soft ones
        y.reshape(-1)[::4] = np.array([0.0, 1.0, 0.5, 0.25], np.float32)[np.arange(len(y.reshape(-1)[::4])) % 4]
        return y
    return r.randn(B, nl).astype(np.float32)


def run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, labels, beta=0.0, vec=None, eps=None, gamma=None, ignore=None, loss_scale=1.0, old=False):
    """one forward (twice, for loss_run) and one backward inside NaN canaries -> dict of numpy outputs.  old: through mb_head_forward /
    mb_head_backward (the triple) instead of the `_ex` entries"""
    L = _lib.lib()
    code = hl.CODE[kind]
    rows = B + EXTRA_ROWS
    zd = nan_buf(rows * H + GUARD)
    zd[:B * H] = torch.from_numpy(z).reshape(-1).to(DEV)
    Wd, bd = torch.from_numpy(Wc).to(DEV).contiguous(), torch.from_numpy(bc).to(DEV).contiguous()
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32)).reshape(-1).to(DEV)
    vd = None if vec is None else torch.tensor(vec, dtype=torch.float32, device=DEV)
    pooled, logits = nan_buf(rows * H + GUARD), nan_buf(rows * nl + GUARD)
    lossb = nan_buf(2 + GUARD)
    lossb[:2] = 0.0
    lp, lrp = C.c_void_p(lossb.data_ptr()), C.c_void_p(lossb.data_ptr() + 4)
    s = _lib.head_loss_struct(code, beta, None if vd is None else vd.data_ptr(), eps, gamma, ignore)
    if old:
        assert eps is None and gamma is None and ignore is None
        fwd = lambda: _lib.check(L.mb_head_forward(_lib.ptr(zd), _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(lab), _lib.ptr(pooled), _lib.ptr(logits),
                                                   lp, lrp, B, H, nl, None, code, float(beta), _lib.ptr(vd), stream()))
    else:
        fwd = lambda: _lib.check(L.mb_head_forward_ex(_lib.ptr(zd), _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(lab), _lib.ptr(pooled), _lib.ptr(logits),
                                                      lp, lrp, B, H, nl, None, C.byref(s), stream()))
    fwd()
    first = lossb[:2].cpu().numpy().copy()
    lossb[0] = 0.0                           # (the caller clears the step's loss; the running sum goes on)
    fwd()
    dz = torch.full((rows * H + GUARD,), float("nan"), dtype=tdt, device=DEV)
    dWc, dbc, dbp = nan_buf(nl * H + GUARD), nan_buf(nl + GUARD), nan_buf(H + GUARD)
    dWc[:nl * H] = 0.0
    dbc[:nl] = 0.0
    dbp[:H] = 0.0
    if old:
        _lib.check(L.mb_head_backward(dt, None, _lib.ptr(logits), _lib.ptr(lab), float(loss_scale), _lib.ptr(pooled), _lib.ptr(Wd), _lib.ptr(dz),
                                      _lib.ptr(dWc), _lib.ptr(dbc), _lib.ptr(dbp), None, 0, B, H, nl, None, code, float(beta), _lib.ptr(vd), stream()))
    else:
        _lib.check(L.mb_head_backward_ex(dt, None, _lib.ptr(logits), _lib.ptr(lab), float(loss_scale), _lib.ptr(pooled), _lib.ptr(Wd), _lib.ptr(dz),
                                         _lib.ptr(dWc), _lib.ptr(dbc), _lib.ptr(dbp), None, 0, B, H, nl, None, C.byref(s), stream()))
    torch.cuda.synchronize()
    # rows from B upward and everything behind the buffers: untouched; nothing inside is NaN (the dz rows of ignored samples are written)
    for name, t, n in (("pooled", pooled, B * H), ("logits", logits, B * nl), ("dz", dz, B * H), ("dWc", dWc, nl * H), ("dbc", dbc, nl),
                       ("dbp", dbp, H), ("loss", lossb, 2), ("z", zd, B * H)):
        assert bool(torch.isnan(t[n:].float()).all()), "%s: written behind element %d (H %d B %d nl %d %s)" % (name, n, H, B, nl, kind)
        assert not bool(torch.isnan(t[:n].float()).any()), "%s: NaN inside (H %d B %d nl %d %s)" % (name, H, B, nl, kind)
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


@pytest.fixture(scope="module")
def yardstick():
    """kind 0 through the `_ex` entries with a neutral struct: per tensor and dz dtype, the worst error over every (H, B) of the sweep"""
    worst = {}
    for dt, tdt, dn in DTS:
        for H in HS:
            for B in BS + ((65, 130) if H == 256 else ()):
                for nl in (1, 5):
                    z, Wc, bc = inputs(H, B, nl)
                    y = targets("default", B, nl) if nl > 1 else targets("mse", B, 1)[:, 0]
                    got = run_head(H, B, nl, "default", dt, tdt, z, Wc, bc, y)
                    for t, e in errors(got, hl.head_reference(z, Wc, bc, y, "default")).items():
                        worst[(t, dn)] = max(worst.get((t, dn), 0.0), e)
    assert all(v > 0 for v in worst.values()), worst
    yield worst
    path = os.environ.get("MB_HEAD_LOSS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# tests/test_head_loss_options_gpu.py: worst max|got - fp64| / (largest element with every summed term replaced by its magnitude)\n"
                    "# per case, tensor and dz dtype over H in %s, B in %s (+ 65, 130 at H = 256), C in (2, 5), bce at 1 and 3 labels\n" % (HS, BS))
            f.write("# yardstick = kind 0 (MSE at nl = 1, cross entropy at nl = 5) through the _ex entries; bound of an option = 4 x yardstick\n")
            for (t, dn), v in sorted(worst.items()):
                f.write("yardstick                      %-9s %-4s %.3e   bound %.3e\n" % (t, dn, v, 4 * v))
            for (label, t, dn), v in sorted(FIGURES.items()):
                f.write("%-30s %-9s %-4s %.3e\n" % (label, t, dn, v))


def check(label, got, ref, dn, yardstick, labels=None, ignore=None):
    err = errors(got, ref)
    for t, e in err.items():
        FIGURES[(label, t, dn)] = max(FIGURES.get((label, t, dn), 0.0), e)
    for t, e in err.items():
        print("%-30s %-9s %-4s err %.3e  yardstick %.3e" % (label, t, dn, e, yardstick[(t, dn)]))
        assert e <= 4.0 * yardstick[(t, dn)], "%s %s %s: error %.3e > 4 x %.3e" % (label, t, dn, e, yardstick[(t, dn)])
    # the two forwards add the same per-block partial sums with atomics, in whichever order the blocks arrive: each of the nb - 1
    # additions rounds to 2^-24 of a running sum that never exceeds the summed magnitudes, in either run; one block adds once
    nb = (got["dz"].shape[0] + 3) // 4
    assert abs(float(got["loss_first"]) - float(got["loss"])) <= 2 * (nb - 1) * 2.0 ** -24 * ref["scale"]["loss"], (label, got["loss_first"], got["loss"])
    if ignore is not None:                                   # rows of ignored samples: exactly 0 in dz
        rows = np.asarray(labels).reshape(-1) == ignore
        assert not got["dz"][rows].any(), label


def weights(C_):
    return [0.5, 3.0] + [1.0] * (C_ - 2)


def ce_cases(B, C_):
    """(label, labels, options) of the cross entropy at this batch: every case of the module docstring that fits B"""
    y = targets("cross_entropy", B, C_)
    w = weights(C_)
    out = [("ce eps=0.1", y, dict(eps=0.1)), ("ce eps=0.1 weight", y, dict(eps=0.1, vec=w)), ("ce eps=0.5 weight", y, dict(eps=0.5, vec=w))]
    for g in (1.0, 2.0, 3.5):
        out.append(("ce gamma=%g" % g, y, dict(gamma=g)))
    out.append(("ce gamma=2 weight", y, dict(gamma=2.0, vec=w)))
    if B >= 2:
        def ign(rows):
            t = y.copy()
            t[rows] = IGN
            return t
        out += [("ce ignore sample 0", ign([0]), dict(ignore=IGN)), ("ce ignore last sample", ign([B - 1]), dict(ignore=IGN)),
                ("ce ignore last, weight", ign([B - 1]), dict(ignore=IGN, vec=w)),
                ("ce ignore all but one", ign([i for i in range(B) if i != B // 2]), dict(ignore=IGN)),
                ("ce ignore, eps=0.1 weight", ign([0]), dict(ignore=IGN, eps=0.1, vec=w)),
                ("ce ignore, gamma=2", ign([B - 1]), dict(ignore=IGN, gamma=2.0))]
        t = y.copy()
        t[0], t[-1] = 1, 0                                   # an in-range ignore_index: class 1 is a real class, and sample 0 carries it
        out.append(("ce ignore in-range", t, dict(ignore=1, vec=w)))
    if B >= 9:
        t = y.copy()
        t[4:8] = IGN                                         # a whole four-sample block
        out.append(("ce ignore a whole block", t, dict(ignore=IGN)))
        t = y.copy()
        t[::2] = IGN
        out.append(("ce ignore every other", t, dict(ignore=IGN, eps=0.1)))
    return out


def run_case(H, B, nl, kind, dt, tdt, dn, yardstick, label, y, opt, loss_scale=1.0):
    z, Wc, bc = inputs(H, B, nl)
    got = run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, y, loss_scale=loss_scale, **opt)
    ref = ho.head_reference(z, Wc, bc, y, kind, vec=opt.get("vec"), loss_scale=loss_scale, smoothing=opt.get("eps") or 0.0,
                            ignore=opt.get("ignore"), gamma=opt.get("gamma") or 0.0)
    check(label, got, ref, dn, yardstick, labels=y, ignore=opt.get("ignore"))
    return got


@pytest.mark.parametrize("dt,tdt,dn", DTS)
@pytest.mark.parametrize("H", HS)
def test_options_against_fp64(yardstick, H, dt, tdt, dn):
    for B in BS + ((65, 130) if H == 256 else ()):
        for C_ in (2, 5):
            for label, y, opt in ce_cases(B, C_):
                run_case(H, B, C_, "cross_entropy", dt, tdt, dn, yardstick, label, y, opt, loss_scale=1.0 if B != 5 else 0.5)
        for nl in (1, 3):
            y = targets("bce", B, nl)
            for g in (1.0, 2.0, 3.5):
                run_case(H, B, nl, "bce", dt, tdt, dn, yardstick, "bce gamma=%g" % g, y, dict(gamma=g))
            run_case(H, B, nl, "bce", dt, tdt, dn, yardstick, "bce gamma=2 pos_weight", y, dict(gamma=2.0, vec=[3.0] if nl == 1 else [0.5, 3.0, 1.0]))


@pytest.mark.parametrize("dt,tdt,dn", DTS)
def test_nothing_kept_is_exactly_zero(dt, tdt, dn):
    """every sample ignored, and a weight of 0 on every kept sample: loss and all four gradient tensors exactly 0, dz written as zeros
    (torch returns NaN here)"""
    for H, B, C_ in ((256, 1, 2), (768, 5, 5), (1024, 9, 5), (256, 65, 2)):
        z, Wc, bc = inputs(H, B, C_)
        w0 = [0.0] + [1.5] * (C_ - 1)
        some = np.zeros(B, np.float32)
        some[1::3] = IGN
        for y, opt in ((np.full(B, IGN, np.float32), dict(ignore=IGN)), (np.full(B, IGN, np.float32), dict(ignore=IGN, eps=0.1, vec=w0)),
                       (np.full(B, IGN, np.float32), dict(ignore=IGN, gamma=2.0)), (np.full(B, 1, np.float32), dict(ignore=1)),
                       (some, dict(ignore=IGN, vec=w0)), (some, dict(ignore=IGN, vec=w0, eps=0.1)), (some, dict(ignore=IGN, vec=w0, gamma=1.0))):
            got = run_head(H, B, C_, "cross_entropy", dt, tdt, z, Wc, bc, y, **opt)
            assert got["loss"] == 0 and got["loss_run"] == 0, (H, B, opt, got["loss"])
            for t in GRADS:
                assert not got[t].any(), (t, H, B, opt)


@pytest.mark.parametrize("dt,tdt,dn", DTS)
def test_neutral_options_give_the_bits_of_the_old_entries(dt, tdt, dn):
    """a neutral mb_head_loss through the `_ex` entries == the old entries, all six kinds; gamma = 0 == the plain kind (one block per
    launch where sums are compared: no atomic meets another)"""
    for H, B in ((256, 4), (768, 3), (1024, 5)):
        one_block = B <= 4
        for nl in (1, 5):
            z, Wc, bc = inputs(H, B, nl)
            for kind in hl.legal_kinds(nl):
                y = targets(kind, B, nl)
                if kind == "default" and nl == 1:
                    y = y[:, 0]
                vec = {"bce": [3.0] if nl == 1 else [0.5, 3.0, 1.0, 1.0, 2.0], "cross_entropy": [0.0, 0.75, 0.75, 0.75, 1.5]}.get(kind)
                beta = 0.3 if kind == "smooth_l1" else 0.0
                a = run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, y, beta=beta, vec=vec, old=True)
                b = run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, y, beta=beta, vec=vec)
                same = ("pooled", "logits", "dz") + (("loss", "dWc", "dbc", "dbp") if one_block else ())
                for t in same:
                    assert np.array_equal(a[t], b[t]), (t, H, B, nl, kind)
                if kind in ("bce", "cross_entropy"):
                    c = run_head(H, B, nl, kind, dt, tdt, z, Wc, bc, y, vec=vec, gamma=0.0, eps=0.0)
                    for t in same:
                        assert np.array_equal(a[t], c[t]), ("gamma = 0", t, H, B, nl, kind)


def test_ignore_without_an_ignored_label_is_the_plain_cross_entropy(yardstick):
    """the kept count of a batch without an ignored label is B, and the weighted form keeps its expressions"""
    dt, tdt, dn = DTS[0]
    for H, B in ((256, 4), (256, 65)):
        z, Wc, bc = inputs(H, B, 5)
        y = targets("cross_entropy", B, 5)
        for vec in (None, weights(5)):
            a = run_head(H, B, 5, "cross_entropy", dt, tdt, z, Wc, bc, y, vec=vec)
            b = run_head(H, B, 5, "cross_entropy", dt, tdt, z, Wc, bc, y, vec=vec, ignore=IGN)
            assert np.array_equal(a["dz"], b["dz"]) and np.array_equal(a["logits"], b["logits"])
            if B <= 4:
                assert a["loss"] == b["loss"] and np.array_equal(a["dWc"], b["dWc"])


def planted(nl, H=256):
    """zero classifier weights: logit k of every sample is bc[k], exactly"""
    return np.random.RandomState(3).randn(1, H).astype(np.float32), np.zeros((nl, H), np.float32)


@pytest.mark.parametrize("big", [88.0, 1e4])
def test_tails_are_finite_and_on_their_limits(yardstick, big):
    dt, tdt, dn = DTS[0]
    f = np.float32
    H = 256
    tiny = 2.0 ** -126
    z, W0 = planted(2)
    bc = np.array([big, -big], f)
    for gamma in (1.0, 2.0, 3.5):
        # focal cross entropy, one sample: p -> 1 (loss 0, gradient 0) and p -> 0 (loss 2 big, gradient (1, -1))
        hit = run_head(H, 1, 2, "cross_entropy", dt, tdt, z, W0, bc, np.array([0], f), gamma=gamma)
        assert np.array_equal(hit["logits"][0], bc) and abs(float(hit["loss"])) < tiny and np.abs(hit["dbc"]).max() < tiny, (gamma, hit["loss"], hit["dbc"])
        miss = run_head(H, 1, 2, "cross_entropy", dt, tdt, z, W0, bc, np.array([1], f), gamma=gamma)
        assert miss["loss"] == f(2 * big) and np.array_equal(miss["dbc"], np.array([1.0, -1.0], f)), (gamma, miss["loss"], miss["dbc"])
        assert not hit["dz"].any() and not miss["dz"].any()              # (zero classifier weights)
    # label smoothing at the same logits: finite, and within the bound of its fp64 value
    for y in (0, 1):
        for vec in (None, [0.5, 3.0]):
            got = run_head(H, 1, 2, "cross_entropy", dt, tdt, z, W0, bc, np.array([y], f), eps=0.1, vec=vec)
            ref = ho.head_reference(z, W0, bc, np.array([y]), "cross_entropy", vec=vec, smoothing=0.1)
            assert np.isfinite(got["loss"]) and np.isfinite(got["dbc"]).all()
            assert abs(float(got["loss"]) - ref["loss"]) <= 4 * yardstick[("loss", dn)] * ref["scale"]["loss"], (got["loss"], ref["loss"])
            assert np.abs(got["dbc"] - ref["dbc"]).max() <= 4 * yardstick[("dbc", dn)] * ref["scale"]["dbc"]
    # sigmoid focal loss: x = (+big, -big, +big, -big) against y = (0, 0, 1, 1): terms (big, 0, 0, big) / 4, gradients (1, 0, 0, -1) / 4
    z, W0 = planted(4)
    bc = np.array([big, -big, big, -big], f)
    y = np.array([[0.0, 0.0, 1.0, 1.0]], f)
    for gamma in (1.0, 2.0, 3.5):
        for vec in (None, [1.0, 3.0, 3.0, 1.0]):                         # (pos_weight on the two entries whose limit is 0)
            got = run_head(H, 1, 4, "bce", dt, tdt, z, W0, bc, y, gamma=gamma, vec=vec)
            assert got["loss"] == f(big / 2), (gamma, got["loss"])
            g = got["dbc"]
            assert g[0] == f(0.25) and g[3] == f(-0.25) and abs(float(g[1])) < tiny and abs(float(g[2])) < tiny, (gamma, g)
        soft = run_head(H, 1, 4, "bce", dt, tdt, z, W0, bc, np.full((1, 4), 0.5, f), gamma=gamma)
        ref = ho.head_reference(z, W0, bc, np.full((1, 4), 0.5), "bce", gamma=gamma)
        assert np.isfinite(soft["loss"]) and np.isfinite(soft["dbc"]).all()
        assert abs(float(soft["loss"]) - ref["loss"]) <= 4 * yardstick[("loss", dn)] * ref["scale"]["loss"]
        assert np.abs(soft["dbc"] - ref["dbc"]).max() <= 4 * yardstick[("dbc", dn)] * ref["scale"]["dbc"]


def test_refusals():
    L = _lib.lib()
    t = torch.zeros(1024, device=DEV)
    p = _lib.ptr(t)

    def fwd(nl, **kw):
        s = _lib.head_loss_struct(**kw)
        return L.mb_head_forward_ex(p, p, p, p, p, p, p, None, 1, 256, nl, None, C.byref(s), stream())

    def bwd(nl, **kw):
        s = _lib.head_loss_struct(**kw)
        return L.mb_head_backward_ex(_lib.DT_F32, None, p, p, 1.0, p, p, p, None, None, None, None, 0, 1, 256, nl, None, C.byref(s), stream())

    for f in (fwd, bwd):
        assert f(2, kind=5, label_smoothing=1.0) == 1004 and f(2, kind=5, label_smoothing=-0.5) == 1004
        assert f(2, kind=5, focal_gamma=0.5) == 1004 and f(2, kind=5, focal_gamma=float("inf")) == 1004 and f(2, kind=4, focal_gamma=float("nan")) == 1004
        assert f(2, kind=5, label_smoothing=0.1, focal_gamma=2.0) == 1004
        assert f(2, kind=4, label_smoothing=0.1) == 1004 and f(2, kind=0, ignore_index=-100) == 1004 and f(2, kind=2, focal_gamma=2.0) == 1004
        assert f(1, kind=5, focal_gamma=2.0) == 1004
    assert L.mb_head_forward_ex(p, p, p, p, p, p, p, None, 1, 256, 2, None, None, stream()) == 1004          # no struct
    torch.cuda.synchronize()
