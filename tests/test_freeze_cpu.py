"""CPU: frozen tensors in the single-call step, host side -- the planner's frozen segments, model.freeze's name sets, the group
builders that leave frozen parameters out, AdamW.flat_step_args' "frozen" key, the driver's flags, and the engines' checks of the
marks (host-only calls: no device needed)."""
import ctypes as C
import os
import re

import pytest
import torch

from bert_multimodal_transformer_amd import AdamW, _lib
from bert_multimodal_transformer_amd import optimization as OPT
from bert_multimodal_transformer_amd.bert import _FusedStep
from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
from bert_multimodal_transformer_amd.optimization import (FROZEN, layerwise_lr_groups, pair_update_groups, plan_paired_segments,
                                                          plan_update_segments)

from test_param_groups_cpu import GROUPS, N_END, TABLE
from test_param_groups_paired_cpu import TableCore, engine_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------- the planner
def test_unowned_runs_become_frozen_segments():
    """layer 0's two weights, the word table and layer 0's bias are in no group: three frozen runs, cut where a neighbour has a group;
    the slot behind the update range is not looked at"""
    owners = list(GROUPS)
    for i in (0, 1, 5, 7):
        owners[i] = None
    got = plan_update_segments(TABLE, owners, N_END, frozen=True)
    assert got == ([0, 5120, 10240, 10496, 11136, 11200, 11264, 11328, 11392, 11520], [FROZEN, 4, 6, FROZEN, 6, FROZEN, 5, 1, 7],
                   [1, 0, 0, 1, 0, 1, 0, 0, 0])
    # consecutive frozen tensors are ONE segment, whatever group they used to have; an empty collection is "no owner" too
    owners[2] = owners[3] = set()
    bounds, classes, flags = plan_update_segments(TABLE, owners, N_END, frozen=True)
    assert bounds[:3] == [0, 10240, 10496] and classes[:2] == [FROZEN, 6] and flags[:2] == [1, 0]
    assert plan_update_segments(TABLE[::-1], owners[::-1], N_END, frozen=True) == (bounds, classes, flags)
    # the slot behind n_update_end may carry anything
    assert plan_update_segments(TABLE, owners[:-1] + [3], N_END, frozen=True) == (bounds, classes, flags)
    # without the switch an unowned tensor is still a reason to decline
    assert plan_update_segments(TABLE, owners, N_END) is None
    # two groups, and everything frozen
    assert plan_update_segments(TABLE, [(0, 1)] + owners[1:], N_END, frozen=True) is None
    assert plan_update_segments(TABLE, [None] * len(TABLE), N_END, frozen=True) is None


def test_frozen_segments_count_towards_the_segment_limit_only():
    n = OPT.UPDATE_SEGMENTS_MAX + 1
    alt = [("t%d" % i, 64 * i, 64) for i in range(n)]
    owners = [0 if i % 2 else None for i in range(n)]
    assert plan_update_segments(alt, owners, 64 * n, frozen=True) is None
    ok = plan_update_segments(alt[:-1], owners[:-1], 64 * (n - 1), frozen=True)
    assert ok is not None and len(ok[1]) == OPT.UPDATE_SEGMENTS_MAX and sum(ok[2]) == OPT.UPDATE_SEGMENTS_MAX // 2
    # 32 classes and a frozen tensor fit (FROZEN is no class), 33 do not
    many = [("t%d" % i, 64 * i, 64) for i in range(34)]
    assert plan_update_segments(many[:33], [None] + list(range(32)), 64 * 33, frozen=True) is not None
    assert plan_update_segments(many, [None] + list(range(33)), 64 * 34, frozen=True) is None


def test_nothing_left_out_plans_as_ever():
    """with every tensor owned the frozen form cuts exactly where today's does, for the plain and the paired planner"""
    plain = plan_update_segments(TABLE, GROUPS, N_END)
    got = plan_update_segments(TABLE, GROUPS, N_END, frozen=True)
    assert got == (plain[0], plain[1], [0] * len(plain[1]))
    hyper = [(1e-3 * (1 + g // 2), (0.9, 0.999), 1e-6, True, 0.0 if g % 2 else 0.01) for g in range(8)]
    class_of, no_decay, _ = pair_update_groups(hyper)
    paired = plan_paired_segments(TABLE, GROUPS, N_END, class_of, no_decay)
    got = plan_paired_segments(TABLE, GROUPS, N_END, class_of, no_decay, frozen=True)
    assert paired is not None and got == paired + ([0] * len(paired[1]),)
    owners = list(GROUPS)
    owners[5] = None
    assert plan_paired_segments(TABLE, owners, N_END, class_of, no_decay) is None
    bounds, classes, flags, frozen = plan_paired_segments(TABLE, owners, N_END, class_of, no_decay, frozen=True)
    assert bounds == paired[0] and frozen == [1 if b == 10496 else 0 for b in bounds[:-1]]
    assert [c for c, f in zip(classes, frozen) if not f] == [c for c, b in zip(paired[1], paired[0]) if b != 10496]


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_real_layouts_plan_the_same_with_nothing_frozen(kind):
    """the two-group and the layer-wise optimizer over a real engine table: flat_step_args is what it was -- no "frozen" key, the same
    map -- compared with the planners' own output on the same input"""
    core = TableCore(kind, 3, 256)
    named = core.named()
    two = AdamW(optimizer_grouped_parameters(_Named(named)), lr=1e-3).flat_step_args(core)
    # (this stand-in core ends its buffer at the last tensor's last element, so the two groups arrive as a two-class map here)
    assert two is not None and "frozen" not in two and two.get("map", ([0, core.n_decay, core.n_update_end], [0, 1])) == \
        ([0, core.n_decay, core.n_update_end], [0, 1])
    opt = AdamW(layerwise_lr_groups(named, 3, 1e-3, layer_decay=0.5, head_lr=5e-3), lr=1e-3)
    args = opt.flat_step_args(core)
    owner = {p._mb_flat[1]: gi for gi, g in enumerate(opt.param_groups) for p in g["params"] if hasattr(p, "_mb_flat")}
    plain = plan_update_segments(core.tensors, [owner.get(t[1]) for t in core.tensors], core.n_update_end)
    groups = sorted(set(plain[1]))
    assert "frozen" not in args and args["map"] == (plain[0], [groups.index(g) for g in plain[1]])


class _Named(torch.nn.Module):
    def __init__(self, named):
        super().__init__()
        self._named = named

    def named_parameters(self, *a, **k):
        return iter(self._named)


# ------------------------------------------------------------------------------------------------------------------ model.freeze
class _Stub(_FusedStep, torch.nn.Module):
    """model.freeze / unfreeze over the real parameter names of an engine layout (no device: the parameters are placeholders)"""

    def __init__(self, kind, layers):
        torch.nn.Module.__init__(self)
        self.core = TableCore(kind, layers, 256)
        self._core = type("Core", (), {"n_layers": layers})()
        self._named = self.core.named()

    def named_parameters(self, *a, **k):
        return iter(self._named)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_freeze_names(kind):
    m = _Stub(kind, 4)
    every = [n for n, _ in m.named_parameters()]
    layer = lambda l: [n for n in every if ("encoder.layer.%d." % l) in n or ("transformer.layer.%d." % l) in n]
    assert m.freeze() == [] and all(p.requires_grad for _, p in m.named_parameters())
    got = m.freeze(layers=2)
    assert got == sorted(layer(0) + layer(1)) and len(layer(0)) == (16 if kind == "bert" else 17)
    assert {n for n, p in m.named_parameters() if not p.requires_grad} == set(got)
    assert m.unfreeze() == got and all(p.requires_grad for _, p in m.named_parameters())
    emb = m.freeze(embeddings=True, layers=(3,))
    if kind == "bert":
        want_emb = ["bert.embeddings.LayerNorm.bias", "bert.embeddings.LayerNorm.weight", "bert.embeddings.position_embeddings.weight",
                    "bert.embeddings.token_type_embeddings.weight", "bert.embeddings.word_embeddings.weight"]
    else:
        want_emb = ["transformer.mask_emb", "transformer.word_embedding.weight"]
    assert emb == sorted(want_emb + layer(3))
    # the gate, the pooler / summary and the heads never freeze
    keep = [n for n in every if any(k in n for k in ("MAG.", "pooler.", "classifier.", "sequence_summary.", "logits_proj."))]
    assert keep and not set(keep) & set(emb)
    with pytest.raises(ValueError):
        m.freeze(layers=5)
    with pytest.raises(ValueError):
        m.freeze(layers=(4,))
    m.unfreeze()


# ------------------------------------------------------------------------------------------------------ groups and flat_step_args
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_groups_drop_frozen_parameters_and_the_step_gets_marks(kind):
    m = _Stub(kind, 3)
    core = m.core
    frozen = set(m.freeze(embeddings=True, layers=2))
    held = lambda groups: {id(p) for g in groups for p in g["params"]}
    by_name = dict(m.named_parameters())
    two = optimizer_grouped_parameters(m)
    assert len(two) == 2 and held(two) == {id(p) for n, p in by_name.items() if n not in frozen}
    lw = layerwise_lr_groups(m.named_parameters(), 3, 1e-3, layer_decay=0.5, head_lr=5e-3)
    assert held(lw) == held(two) and all(g["params"] for g in lw)
    # depths 0 .. 2 are empty now: the groups of layer 2 and of the head are left
    assert len(lw) == 4 and sorted({g["lr"] for g in lw}) == [5e-4, 5e-3]
    for groups, nclasses in ((two, 2), (lw, 4)):
        opt = AdamW(groups, lr=1e-3)
        args = opt.flat_step_args(core)
        assert args is not None and "frozen" in args and len(args["classes"]["lr"]) == nclasses
        bounds, classes = args["map"]
        assert len(args["frozen"]) == len(classes) == len(bounds) - 1 and max(classes) + 1 == nclasses
        marked = set()
        for b, e, f in zip(bounds[:-1], bounds[1:], args["frozen"]):
            for name, off, _ in core.tensors:
                if b <= off < e and f:
                    marked.add(name)
        assert marked == frozen - {"transformer.mask_emb"}          # (MAG-XLNet's slot behind the update range is in no segment)
        # data parallel keeps the Python-driven exchange, as for any map
        opt._dp = object()
        assert opt.flat_step_args(core, allow_dp=True) is None
    # a group emptied by freezing is omitted: every no-decay tensor of this made-up model is frozen
    named = [("a.weight", torch.nn.Parameter(torch.zeros(1))), ("a.bias", torch.nn.Parameter(torch.zeros(1)))]
    assert len(optimizer_grouped_parameters(_Named(named))) == 2
    named[1][1].requires_grad_(False)
    got = optimizer_grouped_parameters(_Named(named))
    assert len(got) == 1 and got[0]["params"][0] is named[0][1] and got[0]["weight_decay"] == 0.01
    assert len(layerwise_lr_groups(named, 1, 1e-3)) == 1
    m.unfreeze()
    assert len(optimizer_grouped_parameters(m)[0]["params"]) + len(optimizer_grouped_parameters(m)[1]["params"]) == len(by_name)


def test_driver_flags():
    from bert_multimodal_transformer_amd import multimodal_driver as D
    a = D.parse_args([])
    assert a.freeze_layers == 0 and a.freeze_embeddings is False
    a = D.parse_args(["--freeze_layers", "6", "--freeze_embeddings"])
    assert a.freeze_layers == 6 and a.freeze_embeddings is True
    assert D.parse_args(["--freeze_embeddings", "false"]).freeze_embeddings is False


# ---------------------------------------------------------------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_marks_need_a_map_and_the_right_count(kind):
    header = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    for name in ("mb_%s_set_update_frozen" % kind, "mb_%s_freeze_stats" % kind):
        assert re.search(r"\b%s\s*\(" % name, header), name
    L = _lib.lib()
    h = C.c_void_p()
    if kind == "bert":
        cfg = _lib.BertEngineConfig(30522, 256, 2, 4, 1024, 512, 2, 1, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_bert_create(C.byref(cfg), C.byref(h)))
    else:
        cfg = _lib.XlnetEngineConfig(32000, 256, 2, 4, 1024, 1, 47, 74, 1, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_xlnet_create(C.byref(cfg), C.byref(h)))
    fn = lambda name: getattr(L, "mb_%s_%s" % (kind, name))
    try:
        rows, end, _ = engine_table(kind, 2, 256)
        one = (C.c_uint8 * 1)(1)
        assert fn("set_update_frozen")(h, 1, one) == 1002                          # no map: MB_ERR_MODE
        second = sorted(r[1] for r in rows)[1]
        bounds, classes = (C.c_size_t * 3)(0, second, end), (C.c_int * 2)(0, 1)
        _lib.check(fn("set_update_map")(h, 2, 2, bounds, classes))
        assert fn("set_update_frozen")(h, 1, one) == 1004                          # a wrong count: MB_ERR_ARG
        assert fn("set_update_frozen")(h, 2, None) == 1004
        _lib.check(fn("set_update_frozen")(h, 2, (C.c_uint8 * 2)(1, 0)))
        elems, wg, emb = C.c_size_t(7), C.c_int(7), C.c_int(7)
        _lib.check(fn("freeze_stats")(h, C.byref(elems), C.byref(wg), C.byref(emb)))
        assert (elems.value, wg.value, emb.value) == (0, 0, 0)                     # no step was enqueued
        _lib.check(fn("set_update_map")(h, 0, 0, None, None))                      # clearing the map clears the marks
        assert fn("set_update_frozen")(h, 2, (C.c_uint8 * 2)(1, 0)) == 1002
    finally:
        fn("destroy")(h)
