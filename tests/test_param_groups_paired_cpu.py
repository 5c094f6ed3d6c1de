"""CPU: paired update classes -- the decayed and the undecayed parameter group of one learning rate share a class slot, and the
segments of the undecayed one carry a no-decay mark (include/magbert_hip.h: mb_*_set_update_decay).  Host side: the pairing pass, the
paired planner, the real layouts of the deep models from the engines' host-only tensor tables, what AdamW.flat_step_args hands to the
step, and the engines' checks of the marks (no device needed)."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from bert_multimodal_transformer_amd import AdamW, _lib
from bert_multimodal_transformer_amd import optimization as OPT
from bert_multimodal_transformer_amd.optimization import (layerwise_lr_groups, pair_update_groups, plan_paired_segments,
                                                          plan_update_segments)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_param_groups_cpu.py's made-up layout: a decay slab with per-layer runs, pooler, word table and classifier weight, then a no-decay
# slab with per-layer runs, and a frozen slot
TABLE = [
    ("enc.layer.0.a.weight", 0, 4096), ("enc.layer.0.b.weight", 4096, 1000),
    ("enc.layer.1.a.weight", 5120, 4096), ("enc.layer.1.b.weight", 9216, 1000),
    ("pooler.weight", 10240, 256), ("emb.word.weight", 10496, 640), ("classifier.weight", 11136, 10),
    ("enc.layer.0.a.bias", 11200, 64), ("enc.layer.1.a.bias", 11264, 64), ("emb.LayerNorm.bias", 11328, 64),
    ("pooler.bias", 11392, 64), ("classifier.bias", 11456, 1),
    ("frozen.slot", 11520, 64),
]
N_END = 11520
# groups as layerwise_lr_groups orders them: embeddings 0 / 1 (decay / no decay), layer 0: 2 / 3, layer 1: 4 / 5, head 6 / 7
GROUPS = [2, 2, 4, 4, 6, 0, 6, 3, 5, 1, 7, 7, None]
B12, EPS = (0.9, 0.999), 1e-6


def hyper(lrs=(1e-3, 2e-3, 3e-3, 4e-3), wd=0.01):
    """(lr, betas, eps, correct_bias, weight_decay) of the eight groups above: one learning rate per depth, decayed then undecayed"""
    return [(lr, B12, EPS, True, w) for lr in lrs for w in (wd, 0.0)]


def test_pairs_found():
    class_of, no_decay, members = pair_update_groups(hyper())
    assert class_of == [0, 0, 1, 1, 2, 2, 3, 3]
    assert no_decay == [False, True] * 4
    assert members == [(0, 1), (2, 3), (4, 5), (6, 7)]
    bounds, classes, flags = plan_paired_segments(TABLE, GROUPS, N_END, class_of, no_decay)
    # the plain planner's boundaries (the two halves of a class never touch here), classes halved, the no-decay slab marked
    plain = plan_update_segments(TABLE, GROUPS, N_END)
    assert bounds == plain[0] == [0, 5120, 10240, 10496, 11136, 11200, 11264, 11328, 11392, 11520]
    assert classes == [g // 2 for g in plain[1]] == [1, 2, 3, 0, 3, 1, 2, 0, 3]
    assert flags == [g % 2 for g in plain[1]] == [0, 0, 0, 0, 0, 1, 1, 1, 1]


@pytest.mark.parametrize("what", ["lr", "betas", "eps", "correct_bias", "both_decay"])
def test_a_pair_is_refused_when_the_groups_disagree(what):
    h = hyper()
    lr, betas, eps, cb, wd = h[3]                        # layer 0's undecayed group
    h[3] = {"lr": (lr * 1.25, betas, eps, cb, wd), "betas": (lr, (0.8, 0.999), eps, cb, wd), "eps": (lr, betas, 1e-8, cb, wd),
            "correct_bias": (lr, betas, eps, False, wd), "both_decay": (lr, betas, eps, cb, 0.02)}[what]
    class_of, no_decay, members = pair_update_groups(h)
    assert class_of == [0, 0, 1, 2, 3, 3, 4, 4]          # groups 2 and 3 stay classes of their own, exactly as without pairing
    assert no_decay == [False, True, False, False, False, True, False, True]
    assert members == [(0, 1), (2, None), (3, None), (4, 5), (6, 7)]


def test_pairing_takes_the_zero_side_wherever_it_stands():
    # the undecayed group first, a lone undecayed group, and two decaying groups of one learning rate with ONE undecayed partner
    h = [(1e-3, B12, EPS, True, 0.0), (1e-3, B12, EPS, True, 0.01), (2e-3, B12, EPS, True, 0.0),
         (3e-3, B12, EPS, True, 0.01), (3e-3, B12, EPS, True, 0.05), (3e-3, B12, EPS, True, 0.0)]
    class_of, no_decay, members = pair_update_groups(h)
    assert class_of == [0, 0, 1, 2, 3, 2]
    assert no_decay == [True, False, False, False, False, True]
    assert members == [(1, 0), (2, None), (3, 5), (4, None)]          # the class carries the decaying group's values


def test_hints_choose_among_equal_partners():
    # a warm-up from lr 0: every group has the same lr, the second depth has no undecayed group -- by index alone depth 1's decayed
    # group would take depth 2's undecayed one; the groups' base learning rates settle it
    h = [(0.0, B12, EPS, True, 0.01), (0.0, B12, EPS, True, 0.0), (0.0, B12, EPS, True, 0.01), (0.0, B12, EPS, True, 0.01), (0.0, B12, EPS, True, 0.0)]
    assert pair_update_groups(h)[2] == [(0, 1), (2, 4), (3, None)]
    assert pair_update_groups(h, hints=[1e-3, 1e-3, 2e-3, 3e-3, 3e-3])[2] == [(0, 1), (2, None), (3, 4)]
    # a hint never forbids a pair: what it leaves over pairs in index order, and None is no hint
    assert pair_update_groups(h, hints=[1e-3, 5e-3, 2e-3, 3e-3, 3e-3])[2] == [(0, 1), (2, None), (3, 4)]
    assert pair_update_groups(h, hints=[None] * 5)[2] == [(0, 1), (2, 4), (3, None)]
    # ... and never makes one: other values, no pair
    h[4] = (1e-4, B12, EPS, True, 0.0)
    assert pair_update_groups(h, hints=[1e-3, 1e-3, 2e-3, 3e-3, 3e-3])[2] == [(0, 1), (2, None), (3, None), (4, None)]


def test_flags_split_a_run_of_one_class():
    # layer 0's bias moved right behind layer 0's weights: one class, two segments
    table = [("l0.w", 0, 4096), ("l0.bias", 4096, 64), ("l1.w", 4160, 1000), ("l1.bias", 5184, 64), ("l1.w2", 5248, 64)]
    groups = [0, 1, 2, 3, 2]
    class_of, no_decay, _ = pair_update_groups(hyper((1e-3, 2e-3)))
    got = plan_paired_segments(table, groups, 5312, class_of, no_decay)
    assert got == ([0, 4096, 4160, 5184, 5248, 5312], [0, 0, 1, 1, 1], [0, 1, 0, 1, 0])
    # without a flag between them consecutive tensors of one class are one segment
    assert plan_paired_segments(table, [0, 0, 2, 2, 2], 5312, class_of, no_decay) == ([0, 4160, 5312], [0, 1], [0, 0])


def test_order_independence():
    class_of, no_decay, _ = pair_update_groups(hyper())
    want = plan_paired_segments(TABLE, GROUPS, N_END, class_of, no_decay)
    assert plan_paired_segments(TABLE[::-1], GROUPS[::-1], N_END, class_of, no_decay) == want
    # the groups in another order: the same segments and marks, and the same tensors share a class
    perm = [5, 2, 7, 0, 3, 6, 1, 4]                      # new index of old group g
    h2 = [None] * 8
    for g, hv in enumerate(hyper()):
        h2[perm[g]] = hv
    c2, nd2, m2 = pair_update_groups(h2)
    got = plan_paired_segments(TABLE, [None if g is None else perm[g] for g in GROUPS], N_END, c2, nd2)
    assert got[0] == want[0] and got[2] == want[2]
    same = lambda cl: [[a == b for b in cl] for a in cl]
    assert same(got[1]) == same(want[1])
    assert sorted(sorted(x for x in pr) for pr in m2) == sorted(sorted((perm[a], perm[b])) for a, b in ((0, 1), (2, 3), (4, 5), (6, 7)))


def test_more_than_the_table_after_pairing_is_still_none():
    n = OPT.UPDATE_CLASSES_MAX + 1
    table = [("t%d" % i, 64 * i, 64) for i in range(2 * n)]
    h = [(1e-3 * (i // 2 + 1), B12, EPS, True, 0.01 if i % 2 == 0 else 0.0) for i in range(2 * n)]
    class_of, no_decay, members = pair_update_groups(h)
    assert len(members) == n == 33
    assert plan_paired_segments(table, list(range(2 * n)), 64 * 2 * n, class_of, no_decay) is None
    class_of, no_decay, members = pair_update_groups(h[:-2])
    ok = plan_paired_segments(table[:-2], list(range(2 * n - 2)), 64 * (2 * n - 2), class_of, no_decay)
    assert ok is not None and len(set(ok[1])) == 32 == OPT.UPDATE_CLASSES_MAX and len(ok[1]) == 64
    # ... and the planner's other refusals hold as in plan_update_segments
    class_of, no_decay, _ = pair_update_groups(hyper())
    partly = list(GROUPS)
    partly[5] = None
    assert plan_paired_segments(TABLE, partly, N_END, class_of, no_decay) is None
    assert plan_paired_segments(TABLE, GROUPS, N_END + 64, class_of, no_decay) is None
    assert plan_paired_segments(TABLE[1:], GROUPS[1:], N_END, class_of, no_decay) is None
    m = OPT.UPDATE_SEGMENTS_MAX + 1
    alt = [("t%d" % i, 64 * i, 64) for i in range(m)]
    assert plan_paired_segments(alt, [i % 2 for i in range(m)], 64 * m, [0, 0], [False, True]) is None
    assert len(plan_paired_segments(alt[:-1], [i % 2 for i in range(m - 1)], 64 * (m - 1), [0, 0], [False, True])[1]) == 128


# ---------------------------------------------------------------------------------------------------------------- the real layouts
@functools.lru_cache(maxsize=None)
def engine_table(kind, layers, hidden):
    """(name, offset, numel) of every tensor of the engine's flat layout, and the end of the update range (host-only calls)"""
    L = _lib.lib()
    h = C.c_void_p()
    heads, inner = hidden // 64, 4 * hidden
    if kind == "bert":
        cfg = _lib.BertEngineConfig(30522, hidden, layers, heads, inner, 512, 2, 1, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_bert_create(C.byref(cfg), C.byref(h)))
    else:
        cfg = _lib.XlnetEngineConfig(32000, hidden, layers, heads, inner, 1, 47, 74, 1, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_xlnet_create(C.byref(cfg), C.byref(h)))
    fn = lambda name: getattr(L, "mb_%s_%s" % (kind, name))
    name = C.create_string_buffer(160)
    off, numel, ndim, decay = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
    shape = (C.c_int64 * 4)()
    rows = []
    for i in range(fn("num_tensors")(h)):
        _lib.check(fn("tensor_info")(h, i, name, 160, C.byref(off), C.byref(numel), C.byref(ndim), shape, C.byref(decay)))
        rows.append((name.value.decode(), off.value, numel.value))
    end = fn("param_count")(h) if kind == "bert" else L.mb_xlnet_trainable_count(h)
    n_decay = fn("decay_count")(h)
    fn("destroy")(h)
    return tuple(rows), end, n_decay


class TableCore(object):
    """what AdamW looks at of a model's flat buffer, laid out by a real engine table; the buffers themselves are never touched"""

    def __init__(self, kind, layers, hidden):
        rows, end, n_decay = engine_table(kind, layers, hidden)
        self.tensors = [r for r in rows]
        self.n_update_end = end
        self.n_params = max(r[1] + r[2] for r in rows)
        self.n_decay = n_decay
        self.sh_begin, self.sh_end = 0, 64
        self.params = self.grads = torch.zeros(1)
        self._adam_m = self._adam_v = torch.zeros(1)

    def named(self):
        out = []
        for name, off, numel in self.tensors:
            p = torch.nn.Parameter(torch.zeros(1))
            if off < self.n_update_end:
                p._mb_flat = (self, off, numel, (numel,))
            out.append((name, p))
        return out


def layerwise_optimizer(kind, layers, hidden, **kw):
    core = TableCore(kind, layers, hidden)
    groups = layerwise_lr_groups(core.named(), layers, 1e-3, layer_decay=0.9, head_lr=5e-3)
    return core, AdamW(groups, lr=1e-3, **kw)


# Segments of the layer-wise map.  MAG-BERT's layout: the layers' GEMM weights, one run per layer; the rest of the decay slab (pooler,
# MAG, embeddings, classifier: 4 runs); the no-decay slab with one run per layer and 3 around them: 2 * layers + 5.  MAG-XLNet keeps a
# layer's seg_embed and layer_norm weights (decayed: the reference's rule names LayerNorm, not layer_norm) apart from its GEMM
# weights, so a layer has two runs in the decay slab and one in the no-decay slab: 3 * layers + 4.  Pairing cuts where the plain planner cuts -- a mark
# only changes where the class changes too, at the border of the two slabs -- so the counts are the layout's own.
@pytest.mark.parametrize("kind,layers,hidden", [("bert", 24, 1024), ("bert", 16, 256), ("xlnet", 24, 1024), ("xlnet", 16, 256)])
def test_deep_layerwise_groups_plan_to_one_class_per_depth(kind, layers, hidden, monkeypatch):
    core, opt = layerwise_optimizer(kind, layers, hidden)
    ngroups = len(opt.param_groups)
    assert ngroups == (2 * (layers + 2) if kind == "bert" else 2 * (layers + 2) - 1) > OPT.UPDATE_CLASSES_MAX
    planned = opt._class_map(core)
    assert planned is not None
    bounds, classes, groups, no_decay, partners = planned
    assert len(set(classes)) == len(groups) == layers + 2 <= OPT.UPDATE_CLASSES_MAX
    nseg = len(classes)
    print("%s %d x %d: %d groups, %d classes, %d segments" % (kind, layers, hidden, ngroups, len(groups), nseg))
    assert nseg == len(no_decay) == len(bounds) - 1 <= OPT.UPDATE_SEGMENTS_MAX
    # the plain planner, its class limit lifted, cuts at the same places: the segment count is the layout's, not the pairing's
    monkeypatch.setattr(OPT, "UPDATE_CLASSES_MAX", 64)
    owner = {p._mb_flat[1]: gi for gi, g in enumerate(opt.param_groups) for p in g["params"] if hasattr(p, "_mb_flat")}
    plain = plan_update_segments(core.tensors, [owner.get(t[1]) for t in core.tensors], core.n_update_end)
    monkeypatch.undo()
    assert plain is not None and plain[0] == bounds and len(plain[1]) == nseg
    assert nseg == (2 * layers + 5 if kind == "bert" else 3 * layers + 4)
    # every segment reads the values of its tensors' own group, but for weight_decay, which the mark settles
    for s, (b, c, f) in enumerate(zip(bounds, classes, no_decay)):
        own, carrier = opt.param_groups[plain[1][s]], opt.param_groups[groups[c]]
        assert all(own[k] == carrier[k] for k in ("lr", "betas", "eps", "correct_bias"))
        assert own["weight_decay"] == (0.0 if f else carrier["weight_decay"])
        assert (b >= core.n_decay) == bool(f)
    # what the step gets
    args = opt.flat_step_args(core)
    assert args["map"] == (bounds, classes) and args["no_decay"] == no_decay and len(args["classes"]["lr"]) == layers + 2
    assert args["classes"]["weight_decay"] == [0.01] * (layers + 2)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_flat_step_args_of_a_16_layer_layerwise_optimizer_returns_a_map(kind):
    """36 (35) groups: more than the class table holds, 18 classes after pairing -- the step stays in the single call"""
    core, opt = layerwise_optimizer(kind, 16, 256, max_grad_norm=1.0)
    args = opt.flat_step_args(core)
    assert args is not None and "map" in args and args["max_grad_norm"] == 1.0
    assert max(args["map"][1]) + 1 == 18 and sum(args["no_decay"]) > 0
    assert len(args["map"][1]) == len(args["no_decay"]) <= OPT.UPDATE_SEGMENTS_MAX


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_twelve_layers_keep_the_plain_planners_map(kind):
    core, opt = layerwise_optimizer(kind, 12, 768)
    owner = {p._mb_flat[1]: gi for gi, g in enumerate(opt.param_groups) for p in g["params"] if hasattr(p, "_mb_flat")}
    plain = plan_update_segments(core.tensors, [owner.get(t[1]) for t in core.tensors], core.n_update_end)
    assert plain is not None
    args = opt.flat_step_args(core)
    used = sorted(set(plain[1]))
    assert args["map"] == (plain[0], [used.index(g) for g in plain[1]]) and "no_decay" not in args
    assert len(args["classes"]["lr"]) == len(opt.param_groups) == (28 if kind == "bert" else 27)
    assert args["classes"]["weight_decay"] == [g["weight_decay"] for g in opt.param_groups]


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_a_warm_up_from_lr_zero_keeps_the_first_plan(kind):
    """get_linear_schedule_with_warmup starts every group at lr 0: the pairs made then are the pairs of the groups' base learning
    rates, so the first real step finds them intact -- the same cached map, no second capture in the engine"""
    from bert_multimodal_transformer_amd import get_linear_schedule_with_warmup
    core, opt = layerwise_optimizer(kind, 16, 256)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    assert all(g["lr"] == 0.0 for g in opt.param_groups)
    first = opt.flat_step_args(core)
    cached = opt._class_maps[id(core)]
    assert len(first["classes"]["lr"]) == 18 and first["classes"]["lr"] == [0.0] * 18
    opt._opt_called = True          # (what the single-call step tells torch's scheduler)
    sch.step()
    second = opt.flat_step_args(core)
    assert opt._class_maps[id(core)] is cached
    assert second["map"] == first["map"] and second["no_decay"] == first["no_decay"]
    assert len(set(second["classes"]["lr"])) == 18 and min(second["classes"]["lr"]) > 0.0


def test_a_broken_pair_is_planned_again():
    core, opt = layerwise_optimizer("bert", 16, 256)
    first = opt.flat_step_args(core)
    assert opt.flat_step_args(core)["map"] == first["map"] and len(first["classes"]["lr"]) == 18
    # a scheduler scales every group alike: the pairs hold, the map is the cached one, the values follow
    for g in opt.param_groups:
        g["lr"] *= 0.5
    again = opt.flat_step_args(core)
    assert again["map"] == first["map"] and again["no_decay"] == first["no_decay"]
    assert again["classes"]["lr"] == [0.5 * x for x in first["classes"]["lr"]]
    cached = opt._class_maps[id(core)]
    # the undecayed half of layer 3 gets a learning rate of its own: it becomes a class of its own, unmarked
    k = next(i for i, g in enumerate(opt.param_groups) if g["weight_decay"] == 0.0 and i == 2 * 4 + 1)
    opt.param_groups[k]["lr"] = 7e-4
    broken = opt.flat_step_args(core)
    assert opt._class_maps[id(core)] is not cached
    assert broken["map"][0] == first["map"][0] and len(broken["classes"]["lr"]) == 19
    assert sum(broken["no_decay"]) == sum(first["no_decay"]) - 1
    assert 7e-4 in broken["classes"]["lr"] and broken["classes"]["weight_decay"].count(0.0) == 1
    # the zero side decays all of a sudden: the same
    opt.param_groups[1]["weight_decay"] = 0.02
    assert len(opt.flat_step_args(core)["classes"]["lr"]) == 20
    # so many broken pairs that the table overflows: the step is driven from Python, as before
    for i, g in enumerate(opt.param_groups):
        if g["weight_decay"] == 0.0:
            g["lr"] = 1e-4 * (i + 1)
    assert opt.flat_step_args(core) is None


# ---------------------------------------------------------------------------------------------------------------------- the C ABI
def test_header_symbols_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    h = C.CDLL(_lib.LIB_PATH)
    for name in ("mb_bert_set_update_decay", "mb_xlnet_set_update_decay"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(h, name), name
        assert name in _lib.PROTOTYPES, name


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_engine_checks_the_marks_on_the_host(kind):
    """mb_*_set_update_decay: NULL engine, no map, another segment count than the map's, NULL marks; the next set_update_map clears
    the marks; the table limits of set_update_map are what they were"""
    L = _lib.lib()
    rows, end, _ = engine_table(kind, 2, 768)
    h = C.c_void_p()
    if kind == "bert":
        cfg = _lib.BertEngineConfig(30522, 768, 2, 12, 3072, 512, 2, 1, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_bert_create(C.byref(cfg), C.byref(h)))
    else:
        cfg = _lib.XlnetEngineConfig(32000, 768, 2, 12, 3072, 1, 47, 74, 1, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_xlnet_create(C.byref(cfg), C.byref(h)))
    fn = lambda name: getattr(L, "mb_%s_%s" % (kind, name))
    offs = sorted(r[1] for r in rows if r[1] < end)
    set_map = lambda nc, b, c: fn("set_update_map")(h, nc, len(c), (C.c_size_t * len(b))(*b), (C.c_int * len(c))(*c))
    marks = lambda xs: fn("set_update_decay")(h, len(xs), (C.c_uint8 * len(xs))(*xs))
    ARG, MODE = 1004, 1002
    assert fn("set_update_decay")(None, 2, (C.c_uint8 * 2)(0, 1)) == ARG          # NULL engine
    assert marks([0, 1]) == MODE                                                  # no map installed
    assert set_map(1, [0, offs[3], end], [0, 0]) == 0
    assert marks([0, 1, 0]) == ARG and marks([1]) == ARG                          # another segment count than the map's
    assert fn("set_update_decay")(h, 2, None) == ARG
    assert marks([0, 1]) == 0 and marks([0, 1]) == 0 and marks([0, 7]) == 0       # (any non-zero byte is a mark)
    # values belong to the classes, not to the marks: one class here
    fl = lambda n, v: (C.c_float * n)(*([v] * n))
    vals = lambda n: fn("set_update_values")(h, n, fl(n, 1e-3), fl(n, 0.9), fl(n, 0.999), fl(n, 1e-6), fl(n, 0.01), (C.c_int * n)(*([1] * n)))
    assert vals(2) == ARG and vals(1) == 0
    # the same map again clears the marks (so the marks can be set anew), a cleared map takes none
    assert set_map(1, [0, offs[3], end], [0, 0]) == 0 and marks([1, 0]) == 0
    assert set_map(33, [0, offs[3], end], [0, 1]) == ARG                          # the class table is as large as it was
    assert fn("set_update_map")(h, 0, 0, None, None) == 0
    assert marks([0, 1]) == MODE
    fn("destroy")(h)
