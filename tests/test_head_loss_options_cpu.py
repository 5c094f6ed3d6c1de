"""The head-loss options without a GPU: the fp64 helper the GPU tests expect from (tests/head_loss_options_helpers.py) against
torch.nn.functional with autograd in fp64, what make_loss / check_labels / torch_loss accept and apply, and the engines' `_ex` setter
and getter (checked before any device call, so an engine that was only created will do)."""
import ctypes as C
import itertools
import math
import types

import numpy as np
import pytest
import torch

import head_loss_helpers as hl
import head_loss_options_helpers as ho
from bert_multimodal_transformer_amd import _lib, losses

F = torch.nn.functional
ERR_ARG = 1004


# ---------------------------------------------------------------------------------------------- the fp64 helper against torch
def _torch_ce(x, y, vec, smoothing, ignore):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    v = None if vec is None else torch.tensor(vec, dtype=torch.float64)
    loss = F.cross_entropy(xt, torch.tensor(y, dtype=torch.int64), weight=v, ignore_index=-100 if ignore is None else ignore,
                           label_smoothing=smoothing)
    loss.backward()
    return float(loss.detach()), xt.grad.numpy()


def _close(got, want, what):
    got_l, got_g = got
    want_l, want_g = want
    assert math.isfinite(got_l) and np.isfinite(got_g).all(), what
    assert abs(got_l - want_l) <= 1e-13 * max(1.0, abs(want_l)), (what, got_l, want_l)
    assert np.abs(got_g - want_g).max() <= 1e-14 * max(1.0, np.abs(want_g).max()), (what, np.abs(got_g - want_g).max())


@pytest.mark.parametrize("nl", [2, 5])
def test_helper_cross_entropy_matches_torch(nl):
    r = np.random.RandomState(40 + nl)
    w = r.rand(nl) + 0.5
    for B in (1, 4, 9):
        for big in (False, True):
            x = r.randn(B, nl) * 2.0
            if big:                                              # logits also at +-88
                x[0, 0], x[0, -1] = 88.0, -88.0
                x[-1, 0], x[-1, -1] = -88.0, 88.0
            for vec, eps, ignore in itertools.product((None, w), (0.0, 0.1, 0.5), (None, -100, 1)):
                y = r.randint(0, nl, size=B)
                y[0] = 0                                         # one kept sample whatever is ignored
                if ignore == -100 and B > 1:
                    y[1::2] = -100
                if ignore == 1 and B > 1:
                    y[-1] = 1                                    # an in-range index that names a real class
                got = ho.loss_and_grad("cross_entropy", x, y, vec=vec, smoothing=eps, ignore=ignore)
                _close(got, _torch_ce(x, y, vec, eps, ignore), (nl, B, big, vec is not None, eps, ignore))
                if ignore is not None:
                    assert not got[1][y == ignore].any()         # the gradient of an ignored sample: exactly 0


def test_helper_w_zero_convention():
    x = np.random.RandomState(3).randn(4, 3)
    for kw in (dict(ignore=-100), dict(ignore=-100, smoothing=0.1), dict(ignore=-100, gamma=2.0), dict(ignore=2, vec=[1.0, 2.0, 3.0])):
        y = np.full(4, kw["ignore"])
        l, g = ho.loss_and_grad("cross_entropy", x, y, **kw)
        assert l == 0.0 and not g.any(), kw
    # every kept sample in a class of weight 0
    y = np.array([0, 0, -100, 0])
    for kw in (dict(), dict(smoothing=0.1), dict(gamma=2.0)):
        l, g = ho.loss_and_grad("cross_entropy", x, y, vec=[0.0, 1.0, 2.0], ignore=-100, **kw)
        assert l == 0.0 and not g.any(), kw
    assert ho.loss_magnitude("cross_entropy", x, y, vec=[0.0, 1.0, 2.0], ignore=-100) == 0.0


def _torch_focal_ce(x, y, vec, gamma, ignore):
    """the formula of the issue with torch ops: sum_kept w[y] (1 - p)^gamma (-log p) / W"""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.int64)
    keep = torch.ones_like(yt, dtype=torch.bool) if ignore is None else yt != ignore
    ys = torch.where(keep, yt, torch.zeros_like(yt))
    logq = torch.log_softmax(xt, dim=1)
    logp = logq.gather(1, ys[:, None])[:, 0]
    w = torch.ones(x.shape[1], dtype=torch.float64) if vec is None else torch.tensor(vec, dtype=torch.float64)
    wy = w[ys] * keep.double()
    loss = (wy * (1.0 - logp.exp()).pow(gamma) * -logp).sum() / wy.sum()
    loss.backward()
    return float(loss.detach()), xt.grad.numpy()


@pytest.mark.parametrize("gamma", [1.0, 2.0, 3.5])
def test_helper_focal_matches_autograd(gamma):
    r = np.random.RandomState(int(10 * gamma))
    for nl in (2, 5):
        w = r.rand(nl) + 0.5
        for B in (1, 5):
            x = r.randn(B, nl) * 2.0
            y = r.randint(0, nl, size=B)
            for vec, ignore in ((None, None), (w, None), (w, -100), (None, 1)):
                yy = y.copy()
                yy[0] = 0
                if ignore is not None and B > 1:
                    yy[-1] = ignore
                _close(ho.loss_and_grad("cross_entropy", x, yy, vec=vec, gamma=gamma, ignore=ignore), _torch_focal_ce(x, yy, vec, gamma, ignore),
                       ("ce", gamma, nl, B))
    # sigmoid focal loss on bce's term, soft targets included
    for nl in (1, 3):
        x = r.randn(4, nl) * 2.0
        y = r.rand(4, nl)
        y[0, 0], y[1, -1] = 0.0, 1.0
        for vec in (None, list(np.linspace(0.5, 3.0, nl))):
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            yt = torch.tensor(y, dtype=torch.float64)
            v = None if vec is None else torch.tensor(vec, dtype=torch.float64)
            m = yt * torch.sigmoid(-xt) + (1.0 - yt) * torch.sigmoid(xt)
            loss = (m.pow(gamma) * F.binary_cross_entropy_with_logits(xt, yt, pos_weight=v, reduction="none")).mean()
            loss.backward()
            _close(ho.loss_and_grad("bce", x, y, vec=vec, gamma=gamma), (float(loss.detach()), xt.grad.numpy()), ("bce", gamma, nl))


def test_helper_gamma_zero_and_tails():
    r = np.random.RandomState(8)
    x, y = r.randn(5, 3), r.randint(0, 3, size=5)
    w = [0.5, 1.0, 2.0]
    for vec in (None, w):
        a, b = ho.loss_and_grad("cross_entropy", x, y, vec=vec, gamma=0.0), hl.loss_and_grad("cross_entropy", x, y, vec=vec)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    t = r.rand(5, 3)
    a, b = ho.loss_and_grad("bce", x, t, vec=w, gamma=0.0), hl.loss_and_grad("bce", x, t, vec=w)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    # the tails: logits at +-88 and +-1e4 stay finite and sit on their limits
    for big in (88.0, 1e4):
        xb = np.array([[big, -big], [big, -big]])
        for gamma in (1.0, 2.0, 3.5):
            l, g = ho.loss_and_grad("cross_entropy", xb, np.array([0, 1]), gamma=gamma)
            assert math.isfinite(l) and np.isfinite(g).all()
            assert abs(l - big) <= 1e-12 * big                       # sample 0 (p -> 1): 0; sample 1 (p -> 0): 2 big, over W = 2
            assert np.abs(g[0]).max() < 1e-30 and np.abs(g[1] - np.array([0.5, -0.5])).max() < 1e-30
            l, g = ho.loss_and_grad("bce", np.array([[big, -big, big, -big]]), np.array([[0.0, 0.0, 1.0, 1.0]]), gamma=gamma)
            assert abs(l - 2 * big / 4) < 1e-30 and np.abs(g[0] - np.array([0.25, 0.0, 0.0, -0.25])).max() < 1e-30
    # gamma = 1 where 1 - p == 0 exactly: the power is 1, not 0 * inf
    l, g = ho.loss_and_grad("cross_entropy", np.array([[1e4, -1e4]]), np.array([0]), gamma=1.0)
    assert l == 0.0 and not g.any()


def test_head_reference_with_options_matches_autograd():
    r = np.random.RandomState(5)
    B, H, nl = 5, 16, 3
    z, Wc, bc = r.randn(B, H), r.randn(nl, H) * 0.3, r.randn(nl)
    mask = (r.rand(B, H) > 0.2) / 0.8
    y = np.array([0, -100, 2, 1, -100])
    w = [0.5, 1.0, 3.0]
    ref = ho.head_reference(z, Wc, bc, y, "cross_entropy", vec=w, mask=mask, loss_scale=0.5, smoothing=0.1, ignore=-100)
    zt, Wt, bt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (z, Wc, bc))
    pooled = torch.tanh(zt)
    logits = (pooled * torch.tensor(mask)) @ Wt.t() + bt
    loss = F.cross_entropy(logits, torch.tensor(y), weight=torch.tensor(w, dtype=torch.float64), ignore_index=-100, label_smoothing=0.1)
    (0.5 * loss).backward()
    assert abs(ref["loss"] - float(loss.detach())) < 1e-14
    for key, t in (("dz", zt.grad), ("dWc", Wt.grad), ("dbc", bt.grad)):
        assert np.abs(ref[key] - t.numpy()).max() < 1e-14, key
    assert not ref["dz"][y == -100].any() and ref["scale"]["loss"] >= abs(ref["loss"]) > 0


# ---------------------------------------------------------------------------------------------- losses.py
def test_make_loss_options_and_refusals():
    got = losses.make_loss("cross_entropy", 3, weight=[0.0, 1.0, 2.0], label_smoothing=0.1, ignore_index=-100)
    assert (got.label_smoothing, got.ignore_index, got.focal_gamma, got.vector) == (0.1, -100, None, (0.0, 1.0, 2.0))
    assert repr(got) == "HeadLoss('cross_entropy', weight=(0.0, 1.0, 2.0), label_smoothing=0.1, ignore_index=-100)"
    got = losses.make_loss("bce", 3, focal_gamma=2)
    assert (got.focal_gamma, got.label_smoothing, got.ignore_index) == (2.0, None, None) and repr(got) == "HeadLoss('bce', focal_gamma=2.0)"
    assert losses.make_loss("cross_entropy", 3, ignore_index=1).ignore_index == 1                 # an in-range index is legal
    assert losses.make_loss("cross_entropy", 3, focal_gamma=3.5, ignore_index=np.int64(7)).ignore_index == 7
    # neutral values are "not set": the same object as without them, and HeadLoss() is still the default
    assert losses.make_loss("cross_entropy", 3, label_smoothing=0.0, focal_gamma=0) == losses.make_loss("cross_entropy", 3)
    assert losses.make_loss("cross_entropy", 3, label_smoothing=0.1) != losses.make_loss("cross_entropy", 3)
    assert losses.HeadLoss() == losses.make_loss("default", 1) and repr(losses.HeadLoss()) == "HeadLoss('default')"
    bad = [("cross_entropy", dict(label_smoothing=1.0)), ("cross_entropy", dict(label_smoothing=-0.1)),
           ("cross_entropy", dict(label_smoothing=float("nan"))), ("cross_entropy", dict(focal_gamma=0.5)),
           ("cross_entropy", dict(focal_gamma=-1.0)), ("cross_entropy", dict(focal_gamma=float("inf"))),
           ("cross_entropy", dict(focal_gamma=float("nan"))), ("cross_entropy", dict(label_smoothing=0.1, focal_gamma=2.0)),
           ("cross_entropy", dict(ignore_index=1.5)), ("cross_entropy", dict(ignore_index=True)), ("cross_entropy", dict(ignore_index="x")),
           ("bce", dict(label_smoothing=0.1)), ("bce", dict(ignore_index=-100)), ("bce", dict(focal_gamma=0.25)),
           ("default", dict(ignore_index=-100)), ("default", dict(label_smoothing=0.1)), ("default", dict(focal_gamma=2.0)),
           ("mse", dict(focal_gamma=2.0)), ("l1", dict(label_smoothing=0.1)), ("smooth_l1", dict(ignore_index=0))]
    for name, kw in bad:
        with pytest.raises(ValueError) as err:
            losses.make_loss(name, 3, **kw)
        assert all(k in str(err.value) for k in hl.KINDS), (name, kw, str(err.value))


def test_check_labels_with_ignore_index():
    plain = losses.make_loss("cross_entropy", 3)
    ign = losses.make_loss("cross_entropy", 3, ignore_index=-100)
    inr = losses.make_loss("cross_entropy", 3, ignore_index=1, focal_gamma=2.0)
    y = torch.tensor([0.0, -100.0, 2.0, 1.0])
    losses.check_labels(ign, y, 4, 3)
    losses.check_labels(ign, y.long(), 4, 3)
    losses.check_labels(inr, torch.tensor([1, 1, 0, 2]), 4, 3)
    for loss in (plain, losses.make_loss("default", 3), inr):                        # -100 where it is not the configured index
        with pytest.raises(ValueError, match="class indices"):
            losses.check_labels(loss, y, 4, 3)
    for bad in (torch.tensor([0.0, -100.0, 3.0, 1.0]), torch.tensor([0.0, -100.0, 0.5, 1.0]), torch.tensor([0.0, -100.0, -1.0, 1.0])):
        with pytest.raises(ValueError, match="class indices"):
            losses.check_labels(ign, bad, 4, 3)
    with pytest.raises(ValueError, match="every label"):
        losses.check_labels(ign, torch.full((4,), -100.0), 4, 3)
    with pytest.raises(ValueError, match="every label"):
        losses.check_labels(inr, torch.tensor([1, 1, 1, 1]), 4, 3)
    with pytest.raises(ValueError, match="labels"):
        losses.check_labels(ign, y[:3], 4, 3)
    # through _Core._inputs, as every pass goes: refused on the host, before any device is touched
    from bert_multimodal_transformer_amd.bert import _Core
    core = types.SimpleNamespace(config=types.SimpleNamespace(num_labels=3), device=torch.device("cpu"), loss=ign)
    with pytest.raises(ValueError, match="every label"):
        _Core._inputs(core, torch.zeros(4, 8, dtype=torch.int64), None, None, None, None, torch.full((4,), -100))


def test_torch_loss_applies_the_options():
    r = np.random.RandomState(12)
    x = r.randn(6, 5)
    xt = lambda: torch.tensor(x, dtype=torch.float64, requires_grad=True)
    w = (0.0, 1.5, 0.5, 1.0, 2.0)
    y = np.array([4, -100, 2, 1, -100, 3])
    cases = [(dict(label_smoothing=0.1), dict(smoothing=0.1), np.abs(y) % 5), (dict(ignore_index=-100), dict(ignore=-100), y),
             (dict(weight=w, label_smoothing=0.5, ignore_index=-100), dict(vec=w, smoothing=0.5, ignore=-100), y),
             (dict(ignore_index=3), dict(ignore=3), np.abs(y) % 5), (dict(focal_gamma=2.0), dict(gamma=2.0), np.abs(y) % 5),
             (dict(weight=w, focal_gamma=3.5, ignore_index=-100), dict(vec=w, gamma=3.5, ignore=-100), y),
             (dict(weight=w, focal_gamma=1.0), dict(vec=w, gamma=1.0), np.abs(y) % 5)]
    for kw, hkw, yy in cases:
        loss = losses.make_loss("cross_entropy", 5, **kw)
        t = xt()
        out = losses.torch_loss(loss, t, torch.tensor(yy), 5)
        out.backward()
        _close((float(out.detach()), t.grad.numpy()), ho.loss_and_grad("cross_entropy", x, yy, **hkw), kw)
    tg = r.rand(6, 5)
    for kw, hkw in ((dict(focal_gamma=2.0), dict(gamma=2.0)), (dict(focal_gamma=1.0, pos_weight=(0.5, 3.0, 1.0, 1.0, 2.0)), dict(gamma=1.0, vec=(0.5, 3.0, 1.0, 1.0, 2.0)))):
        t = xt()
        out = losses.torch_loss(losses.make_loss("bce", 5, **kw), t, torch.tensor(tg), 5)
        out.backward()
        _close((float(out.detach()), t.grad.numpy()), ho.loss_and_grad("bce", x, tg, **hkw), kw)
    # W == 0: a zero with zero gradients, not torch's NaN -- every sample ignored, and every kept sample at weight 0
    for kw, yy in ((dict(ignore_index=-100), np.full(6, -100)), (dict(ignore_index=-100, label_smoothing=0.1), np.full(6, -100)),
                   (dict(ignore_index=-100, focal_gamma=2.0), np.full(6, -100)), (dict(weight=w), np.zeros(6, np.int64)),
                   (dict(weight=w, ignore_index=-100, label_smoothing=0.1), np.array([0, -100, 0, 0, -100, 0])),
                   (dict(weight=w, focal_gamma=2.0), np.zeros(6, np.int64))):
        t = xt()
        out = losses.torch_loss(losses.make_loss("cross_entropy", 5, **kw), t, torch.tensor(yy), 5)
        out.backward()
        assert float(out.detach()) == 0.0 and not t.grad.numpy().any(), kw
    # without options: what it always was
    t = xt()
    assert float(losses.torch_loss(losses.make_loss("cross_entropy", 5), t, torch.tensor(np.abs(y) % 5), 5)) == \
        float(F.cross_entropy(t, torch.tensor(np.abs(y) % 5)))


# ---------------------------------------------------------------------------------------------- the engines' _ex entries
def _bert_cfg(nl):
    return _lib.BertEngineConfig(30522, 256, 2, 4, 1024, 512, 2, nl, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_F32, 4, 50, 0)


def _xlnet_cfg(nl):
    return _lib.XlnetEngineConfig(32000, 256, 2, 4, 1024, nl, 47, 74, 1, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_F32, 4, 50, 0)


class _Engine(object):
    def __init__(self, model, nl):
        L = _lib.lib()
        self.nl = nl
        self.fn = lambda name: getattr(L, "mb_%s_%s" % (model, name))
        self.h = C.c_void_p()
        cfg = _bert_cfg(nl) if model == "bert" else _xlnet_cfg(nl)
        _lib.check(self.fn("create")(C.byref(cfg), C.byref(self.h)))

    def set_ex(self, kind, param=0.0, vec=None, eps=None, gamma=None, ignore=None):
        arr = None if vec is None else (C.c_float * len(vec))(*vec)
        s = _lib.head_loss_struct(kind, param, None if arr is None else C.addressof(arr), eps, gamma, ignore)
        return self.fn("set_head_loss_ex")(self.h, C.byref(s))

    def get_ex(self):
        """(kind, param, vec, eps, gamma, ignore or None)"""
        s, has = _lib.HeadLossStruct(-1, -1.0, None, -1.0, -1.0, -1, -1), C.c_int(-1)
        vec = (C.c_float * self.nl)(*([-1.0] * self.nl))
        _lib.check(self.fn("get_head_loss_ex")(self.h, C.byref(s), vec, C.byref(has)))
        assert s.vec is None
        return (s.kind, s.param, tuple(vec) if has.value else None, round(s.label_smoothing, 6), s.focal_gamma,
                s.ignore_index if s.has_ignore_index else None)

    def get(self):
        kind, param, has = C.c_int(-1), C.c_float(-1.0), C.c_int(-1)
        vec = (C.c_float * self.nl)(*([-1.0] * self.nl))
        _lib.check(self.fn("get_head_loss")(self.h, C.byref(kind), C.byref(param), vec, C.byref(has)))
        return kind.value, param.value, (tuple(vec) if has.value else None)

    def close(self):
        self.fn("destroy")(self.h)


@pytest.mark.parametrize("model", ["bert", "xlnet"])
def test_ex_setter_validation_and_getter(model):
    e1, e3 = _Engine(model, 1), _Engine(model, 3)
    try:
        before = (e1.fn("workspace_bytes")(e1.h), e3.fn("workspace_bytes")(e3.h))
        assert e3.get_ex() == (0, 0.0, None, 0.0, 0.0, None)                         # an engine starts neutral
        assert e3.set_ex(5, vec=[0.0, 1.0, 2.0], eps=0.25, ignore=-100) == 0
        held = (5, 0.0, (0.0, 1.0, 2.0), 0.25, 0.0, -100)
        assert e3.get_ex() == held
        nan, inf = float("nan"), float("inf")
        for eps in (-0.1, 1.0, 1.5, nan, inf):                                       # eps outside [0, 1)
            assert e3.set_ex(5, eps=eps) == ERR_ARG
        for gamma in (-1.0, 0.5, 0.999, nan, inf, -inf):                             # gamma not in {0} u [1, inf)
            assert e3.set_ex(5, gamma=gamma) == ERR_ARG and e3.set_ex(4, gamma=gamma) == ERR_ARG
        assert e3.set_ex(5, eps=0.1, gamma=2.0) == ERR_ARG                           # both
        for kind in (0, 1, 2, 3, 4):                                                 # smoothing / ignore_index belong to cross_entropy
            assert e3.set_ex(kind, eps=0.1) == ERR_ARG and e3.set_ex(kind, ignore=-100) == ERR_ARG and e3.set_ex(kind, ignore=0) == ERR_ARG
        for kind in (0, 1, 2, 3):                                                    # gamma to cross_entropy and bce
            assert e3.set_ex(kind, gamma=2.0) == ERR_ARG
        assert e1.set_ex(5, eps=0.1) == ERR_ARG                                      # cross entropy needs two classes
        assert e3.set_ex(6) == ERR_ARG and e3.set_ex(-1) == ERR_ARG
        assert e3.set_ex(5, vec=[0.0, 0.0, 0.0], eps=0.1) == ERR_ARG and e3.set_ex(3, param=-1.0) == ERR_ARG       # the triple's own checks
        assert e3.fn("set_head_loss_ex")(e3.h, None) == ERR_ARG
        assert e3.get_ex() == held                                                   # refused: what was set stays
        # round trips
        for args, want in ((dict(kind=5, gamma=1.0), (5, 0.0, None, 0.0, 1.0, None)), (dict(kind=5, gamma=3.5, ignore=2), (5, 0.0, None, 0.0, 3.5, 2)),
                           (dict(kind=5, eps=0.5, ignore=0), (5, 0.0, None, 0.5, 0.0, 0)), (dict(kind=4, vec=[0.5, 1.0, 3.0], gamma=2.0), (4, 0.0, (0.5, 1.0, 3.0), 0.0, 2.0, None)),
                           (dict(kind=5, gamma=0.0, eps=0.0), (5, 0.0, None, 0.0, 0.0, None)), (dict(kind=3, param=0.25), (3, 0.25, None, 0.0, 0.0, None))):
            assert e3.set_ex(**args) == 0 and e3.get_ex() == want, args
        assert e1.set_ex(4, vec=[2.0], gamma=2.0) == 0 and e1.get_ex() == (4, 0.0, (2.0,), 0.0, 2.0, None)
        # the old getter reads the triple; the old setter clears the options
        assert e3.set_ex(5, vec=[1.0, 1.0, 2.0], eps=0.1, ignore=-100) == 0 and e3.get() == (5, 0.0, (1.0, 1.0, 2.0))
        arr = (C.c_float * 3)(1.0, 1.0, 2.0)
        assert e3.fn("set_head_loss")(e3.h, 5, 0.0, arr) == 0
        assert e3.get_ex() == (5, 0.0, (1.0, 1.0, 2.0), 0.0, 0.0, None)
        assert e3.set_ex(4, gamma=2.0) == 0 and e3.fn("set_head_loss")(e3.h, 4, 0.0, None) == 0 and e3.get_ex() == (4, 0.0, None, 0.0, 0.0, None)
        assert (e1.fn("workspace_bytes")(e1.h), e3.fn("workspace_bytes")(e3.h)) == before
    finally:
        e1.close()
        e3.close()


def test_struct_layout_and_configs():
    """mb_head_loss is 32 bytes with the pointer at 8; the config structs keep their last field"""
    assert C.sizeof(_lib.HeadLossStruct) == 32 and _lib.HeadLossStruct.vec.offset == 8 and _lib.HeadLossStruct.ignore_index.offset == 28
    assert _lib.BertEngineConfig._fields_[-1][0] == "hidden_act" and _lib.XlnetEngineConfig._fields_[-1][0] == "ff_activation"
