"""Head losses without a GPU: the engines' setter / getter (checked before any device call, so an engine that was only created will do),
what set_loss and _inputs refuse, and the fp64 helper the GPU tests expect from (tests/head_loss_helpers.py) against
torch.nn.functional with autograd in fp64."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import head_loss_helpers as hl
from bert_multimodal_transformer_amd import _lib, losses

F = torch.nn.functional
ERR_ARG = 1004


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

    def set(self, kind, param=0.0, vec=None):
        arr = None if vec is None else (C.c_float * len(vec))(*vec)
        return self.fn("set_head_loss")(self.h, kind, param, arr)

    def get(self):
        kind, param, has = C.c_int(-1), C.c_float(-1.0), C.c_int(-1)
        vec = (C.c_float * self.nl)(*([-1.0] * self.nl))
        _lib.check(self.fn("get_head_loss")(self.h, C.byref(kind), C.byref(param), vec, C.byref(has)))
        return kind.value, param.value, (tuple(vec) if has.value else None)

    def close(self):
        self.fn("destroy")(self.h)


@pytest.mark.parametrize("model", ["bert", "xlnet"])
def test_setter_validation_and_getter(model):
    e1, e3 = _Engine(model, 1), _Engine(model, 3)
    try:
        before = (e1.fn("workspace_bytes")(e1.h), e3.fn("workspace_bytes")(e3.h))
        assert e1.get() == (0, 0.0, None) and e3.get() == (0, 0.0, None)           # an engine starts with the default kind
        # refused, and what was set stays
        assert e3.set(3, 0.5) == 0
        for e in (e1, e3):
            assert e.set(-1) == ERR_ARG and e.set(6) == ERR_ARG                    # unknown kinds
            for beta in (-0.5, float("nan"), float("inf")):
                assert e.set(3, beta) == ERR_ARG
        assert e1.set(5) == ERR_ARG                                                # cross entropy needs two classes
        for kind in (4, 5):
            for bad in ([1.0, -1.0, 1.0], [1.0, float("nan"), 1.0], [float("inf"), 1.0, 1.0], [0.0, 0.0, 0.0]):
                assert e3.set(kind, 0.0, bad) == ERR_ARG
        assert e3.set(2, 0.0, [1.0, 1.0, 1.0]) == ERR_ARG                          # a vector for a kind that takes none
        assert e3.get() == (3, 0.5, None)
        # every legal kind, and the getter round-trips it
        for kind in range(6):
            assert e3.set(kind, 0.25 if kind == 3 else 0.0) == 0
            assert e3.get() == (kind, 0.25 if kind == 3 else 0.0, None)
        for kind in range(5):
            assert e1.set(kind, 0.0) == 0 and e1.get()[0] == kind
        assert e3.set(3, 0.0) == 0 and e3.get() == (3, 0.0, None)                  # beta == 0 is legal
        assert e3.set(4, 0.0, [0.5, 1.0, 3.0]) == 0 and e3.get() == (4, 0.0, (0.5, 1.0, 3.0))
        assert e3.set(5, 0.0, [0.0, 1.0, 2.0]) == 0 and e3.get() == (5, 0.0, (0.0, 1.0, 2.0))      # a zero among the weights is legal
        assert e1.set(4, 0.0, [2.0]) == 0 and e1.get() == (4, 0.0, (2.0,))
        assert e3.set(0) == 0 and e3.get() == (0, 0.0, None)
        # the workspace plan is not involved
        assert (e1.fn("workspace_bytes")(e1.h), e3.fn("workspace_bytes")(e3.h)) == before
    finally:
        e1.close()
        e3.close()


def test_workspace_bytes_do_not_depend_on_the_loss():
    """the setters exist next to the config structs, which keep their size and their last field"""
    assert _lib.BertEngineConfig._fields_[-1][0] == "hidden_act" and _lib.XlnetEngineConfig._fields_[-1][0] == "ff_activation"
    assert (losses.LOSS_DEFAULT, losses.LOSS_MSE, losses.LOSS_L1, losses.LOSS_SMOOTH_L1, losses.LOSS_BCE, losses.LOSS_CROSS_ENTROPY) == \
        tuple(range(6))
    assert [losses.LOSSES[k] for k in hl.KINDS] == list(range(6))


def test_make_loss_refuses_with_the_six_kinds():
    for name, kw in (("huber", {}), (None, {}), ("l1", {"beta": 1.0}), ("mse", {"pos_weight": [1.0] * 3}), ("bce", {"weight": [1.0] * 3}),
                     ("cross_entropy", {"pos_weight": [1.0] * 3}), ("smooth_l1", {"weight": [1.0] * 3}), ("default", {"beta": 0.5})):
        with pytest.raises(ValueError) as err:
            losses.make_loss(name, 3, **kw)
        assert all(k in str(err.value) for k in hl.KINDS), str(err.value)
    with pytest.raises(ValueError) as err:
        losses.make_loss("cross_entropy", 1)
    assert all(k in str(err.value) for k in hl.KINDS)
    for bad in ([1.0, 2.0], [1.0, -1.0, 1.0], [0.0, 0.0, 0.0], [1.0, float("nan"), 1.0]):
        with pytest.raises(ValueError):
            losses.make_loss("bce", 3, pos_weight=bad)
        with pytest.raises(ValueError):
            losses.make_loss("cross_entropy", 3, weight=bad)
    for beta in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            losses.make_loss("smooth_l1", 3, beta=beta)
    assert losses.make_loss("smooth_l1", 3).beta == 1.0 and losses.make_loss("smooth_l1", 3, beta=0).beta == 0.0
    got = losses.make_loss("bce", 3, pos_weight=torch.tensor([0.5, 1.0, 3.0]))
    assert (got.name, got.code, got.vector, got.per_element) == ("bce", 4, (0.5, 1.0, 3.0), True)
    got = losses.make_loss("cross_entropy", 3, weight=[0.0, 1.0, 2.0])
    assert (got.code, got.vector, got.per_element) == (5, (0.0, 1.0, 2.0), False)
    assert losses.make_loss("default", 1) == losses.HeadLoss() and losses.make_loss("l1", 1) != losses.HeadLoss()


class _FakeCore(object):
    """what _Core._inputs reads before it touches a device"""

    def __init__(self, nl, loss):
        self.config = types.SimpleNamespace(num_labels=nl)
        self.device = torch.device("cpu")
        self.loss = loss


def _inputs(nl, loss, labels, B=4):
    from bert_multimodal_transformer_amd.bert import _Core
    ids = torch.zeros(B, 8, dtype=torch.int64)
    return _Core._inputs(_FakeCore(nl, loss), ids, None, None, None, None, labels)


def test_inputs_checks_labels_per_kind():
    for name in ("mse", "l1", "smooth_l1", "bce"):
        loss = losses.make_loss(name, 3)
        for wrong in (torch.zeros(4), torch.zeros(4, 2), torch.zeros(5, 3)):            # the wrong count for nl = 3
            with pytest.raises(ValueError, match="labels"):
                _inputs(3, loss, wrong)
    bce = losses.make_loss("bce", 3)
    for bad in (1.5, -0.25, float("nan")):
        y = torch.full((4, 3), 0.5)
        y[2, 1] = bad
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            _inputs(3, bce, y)
    for loss in (losses.make_loss("default", 3), losses.make_loss("cross_entropy", 3, weight=[1.0, 2.0, 0.0])):
        for bad in (torch.tensor([0.0, 1.0, 2.0, 3.0]), torch.tensor([0.0, -100.0, 1.0, 2.0]), torch.tensor([0.0, 0.5, 1.0, 2.0])):
            with pytest.raises(ValueError, match="class indices"):                      # a class index equal to nl, ignore_index, a fraction
                _inputs(3, loss, bad)
        with pytest.raises(ValueError, match="labels"):
            _inputs(3, loss, torch.zeros(4, 3))
    with pytest.raises(ValueError, match="labels"):
        _inputs(1, losses.make_loss("default", 1), torch.zeros(3))
    # what passes the checks goes on to the device copies: on this fake core that is an AttributeError on the first tensor, not a ValueError
    for nl, loss, good in ((3, bce, torch.tensor([[0.0, 1.0, 0.5]] * 4)), (3, losses.make_loss("l1", 3), torch.randn(4, 3)),
                           (3, losses.make_loss("cross_entropy", 3), torch.tensor([0, 1, 2, 2])), (1, losses.make_loss("default", 1), torch.randn(4))):
        with pytest.raises(AttributeError):
            _inputs(nl, loss, good)


# ---------------------------------------------------------------------------------------------- the fp64 helper against torch
def _torch_loss_and_grad(kind, x, y, beta=None, vec=None):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    nl = xt.shape[1]
    v = None if vec is None else torch.tensor(vec, dtype=torch.float64)
    kind = hl.resolve(kind, nl)
    if kind == "cross_entropy":
        loss = F.cross_entropy(xt, torch.tensor(np.asarray(y).reshape(-1), dtype=torch.int64), weight=v)
    else:
        yt = torch.tensor(np.asarray(y, np.float64).reshape(x.shape), dtype=torch.float64)
        if kind == "mse":
            loss = F.mse_loss(xt, yt)
        elif kind == "l1":
            loss = F.l1_loss(xt, yt)
        elif kind == "smooth_l1":
            loss = F.smooth_l1_loss(xt, yt, beta=1.0 if beta is None else beta)
        else:
            loss = F.binary_cross_entropy_with_logits(xt, yt, pos_weight=v)
    loss.backward()
    return float(loss.detach()), xt.grad.numpy()


def _agree(kind, x, y, beta=None, vec=None, exact=False):
    want_l, want_g = _torch_loss_and_grad(kind, x, y, beta, vec)
    got_l, got_g = hl.loss_and_grad(kind, x, y, beta=beta, vec=vec)
    assert math.isfinite(got_l) and np.isfinite(got_g).all(), (kind, got_l)
    if exact:
        assert got_l == want_l and np.array_equal(got_g, want_g), (kind, got_l, want_l)
    else:
        assert abs(got_l - want_l) <= 1e-13 * max(1.0, abs(want_l)), (kind, got_l, want_l)
        assert np.abs(got_g - want_g).max() <= 1e-14 * max(1.0, np.abs(want_g).max()), (kind, np.abs(got_g - want_g).max())
    return got_l, got_g


@pytest.mark.parametrize("nl", [1, 2, 5])
def test_helper_matches_torch_on_random_inputs(nl):
    r = np.random.RandomState(7 + nl)
    for B in (1, 3, 9):
        x = r.randn(B, nl) * 2.0
        y = r.randn(B, nl)
        for kind in ("mse", "l1"):
            _agree(kind, x, y)
        for beta in (1.0, 0.3, 2.5):
            _agree("smooth_l1", x, y, beta=beta)
        t = r.rand(B, nl)
        t[0, 0] = 0.0
        t[-1, -1] = 1.0
        _agree("bce", x, t)
        _agree("bce", x, t, vec=np.linspace(0.5, 3.0, nl) if nl > 1 else [0.5])          # pos_weight below and above 1
        _agree("bce", x, t, vec=[3.0] * nl)
        if nl == 1:
            _agree("default", x, y[:, 0])
        else:
            cls = r.randint(0, nl, size=B)
            _agree("default", x, cls)
            _agree("cross_entropy", x, cls)
            w = r.rand(nl) + 0.5
            w[1] = 0.0                                                                       # a weight vector that contains a zero
            cls[0] = 0
            _agree("cross_entropy", x, cls, vec=w)
    # the default kind is mse at one label and the unweighted cross entropy otherwise
    assert hl.resolve("default", 1) == "mse" and hl.resolve("default", 4) == "cross_entropy"
    assert hl.legal_kinds(1) == ["default", "mse", "l1", "smooth_l1", "bce"] and hl.legal_kinds(2) == list(hl.KINDS)


def test_helper_at_the_kinks():
    y = np.array([[0.5, -1.25, 2.0], [0.0, 3.0, -0.75]])
    # d == 0 exactly: gradient exactly 0 for l1 and smooth_l1 (and torch agrees)
    x = y.copy()
    x[1, 2] += 0.5
    for kind, beta in (("l1", None), ("smooth_l1", 1.0), ("smooth_l1", 0.25), ("smooth_l1", 0.0)):
        _, g = _agree(kind, x, y, beta=beta, exact=kind == "l1")
        assert np.array_equal(g[x == y], np.zeros(5)) and g[1, 2] != 0.0
    # |d| == beta exactly: both branches give 0.5 beta and a unit-slope gradient
    for beta in (0.5, 1.0, 2.0):
        x = y + beta * np.array([[1, -1, 1], [-1, 1, -1]])
        l, g = _agree("smooth_l1", x, y, beta=beta)
        assert l == 0.5 * beta and np.array_equal(g * 6, np.sign(x - y))
        inner = y + np.nextafter(beta, 0.0) * np.array([[1, -1, 1], [-1, 1, -1]])
        li, gi = hl.loss_and_grad("smooth_l1", inner, y, beta=beta)
        assert abs(li - l) <= 1e-15 and np.abs(gi - g).max() <= 1e-15
    # beta == 0 is l1, bit for bit
    x = y + np.random.RandomState(3).randn(2, 3)
    x[0, 0] = y[0, 0]
    assert hl.loss_and_grad("smooth_l1", x, y, beta=0.0)[0] == hl.loss_and_grad("l1", x, y)[0]
    assert np.array_equal(hl.loss_and_grad("smooth_l1", x, y, beta=0.0)[1], hl.loss_and_grad("l1", x, y)[1])
    _agree("smooth_l1", x, y, beta=0.0)


def test_helper_bce_limits():
    x = np.array([[1e4, -1e4, 88.0, -88.0]] * 3)
    y = np.array([[0.0] * 4, [1.0] * 4, [0.5] * 4])
    for vec in (None, [0.5, 3.0, 0.5, 3.0]):
        l, g = _agree("bce", x, y, vec=vec)
        p = np.ones(4) if vec is None else np.asarray(vec)
        lw = 1.0 + (p - 1.0) * y
        # at +-1e4 the gradient sits on its limits: (1 - y) / N where the logit is large, -(weight) y ... / N where it is small
        assert np.array_equal(g[:, 0] * 12, 1.0 - y[:, 0]) and np.array_equal(g[:, 1] * 12, (1.0 - y[:, 1]) - lw[:, 1])
        assert np.abs(g[:, 2] * 12 - (1.0 - y[:, 2])).max() < 1e-37 and np.abs(g[:, 3] * 12 - ((1.0 - y[:, 3]) - lw[:, 3])).max() < 1e-37
        assert 0 < l < 1e4


def test_helper_weighted_cross_entropy_edges():
    x = np.random.RandomState(11).randn(5, 3)
    w = [0.0, 1.5, 0.5]
    cls = np.array([0, 1, 0, 2, 1])
    _, g = _agree("cross_entropy", x, cls, vec=w)
    assert np.array_equal(g[cls == 0], np.zeros((2, 3))) and np.abs(g[cls != 0]).min() > 0       # samples of a weight-0 class: gradient 0
    l, g = _agree("cross_entropy", x, np.full(5, 2), vec=w)                                       # all samples share one class
    l1, g1 = hl.loss_and_grad("cross_entropy", x, np.full(5, 2))
    assert abs(l - l1) < 1e-15 and np.abs(g - g1).max() < 1e-16                                   # the weight cancels


def test_head_reference_matches_autograd():
    r = np.random.RandomState(5)
    B, H, nl = 5, 16, 3
    z, Wc, bc = r.randn(B, H), r.randn(nl, H) * 0.3, r.randn(nl)
    mask = (r.rand(B, H) > 0.2) / 0.8
    y = r.rand(B, nl)
    ref = hl.head_reference(z, Wc, bc, y, "bce", vec=[0.5, 1.0, 3.0], mask=mask, loss_scale=0.5)
    zt, Wt, bt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (z, Wc, bc))
    pooled = torch.tanh(zt)
    logits = (pooled * torch.tensor(mask)) @ Wt.t() + bt
    loss = F.binary_cross_entropy_with_logits(logits, torch.tensor(y), pos_weight=torch.tensor([0.5, 1.0, 3.0], dtype=torch.float64))
    (0.5 * loss).backward()
    assert abs(ref["loss"] - float(loss.detach())) < 1e-14
    for key, t in (("dz", zt.grad), ("dWc", Wt.grad), ("dbc", bt.grad)):
        assert np.abs(ref[key] - t.numpy()).max() < 1e-14, key
    assert np.abs(ref["dbp"] - zt.grad.numpy().sum(0)).max() < 1e-14
    assert np.abs(ref["logits"] - logits.detach().numpy()).max() < 1e-14
