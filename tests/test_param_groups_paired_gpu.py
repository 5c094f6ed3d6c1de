"""GPU: layer-wise learning rates on models deeper than 14 layers in the single-call training step.

Layer-wise groups of a 16-layer model are 36 (MAG-XLNet: 35) parameter groups, more than the engines' 32 class slots: the decayed and
the undecayed group of one learning rate share a slot, and the segments of the undecayed one carry a no-decay mark
(include/magbert_hip.h: mb_*_set_update_decay; optimization.pair_update_groups).  The yardstick is the path that takes any groups:
train_step(..., graph=False) = training_step + optimizer.step() with the groups as they are, unpaired; in deterministic mode the
single call equals it bit for bit, as in test_param_groups_gpu.py -- the arithmetic per element is the same, so no tolerance appears
anywhere in this file.  16 layers is the smallest depth that overflows the table; hidden 256 keeps the runs short."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, BertConfig, MAG_BertForSequenceClassification, MAG_XLNetForSequenceClassification,
                                             MultimodalConfig, XLNetConfig, get_linear_schedule_with_warmup, layerwise_lr_groups, _lib)
from oracle import weights

DEV = "cuda:0"
LR, DECAY, HEAD = 1e-3, 0.9, 5e-3
LAYERS = 16
SMALL = ((4, 24),)


def config(kind, hidden, layers, p=0.1):
    if kind == "bert":
        return BertConfig(hidden_size=hidden, num_attention_heads=hidden // 64, intermediate_size=4 * hidden, num_hidden_layers=layers,
                          num_labels=1, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    return XLNetConfig(d_model=hidden, n_head=hidden // 64, d_inner=4 * hidden, n_layer=layers, num_labels=1, dropout=p, summary_last_dropout=p)


@functools.lru_cache(maxsize=None)
def initial_state(kind, hidden, layers):
    """the deterministic test weights of one model size, made once and shared by every twin"""
    cls = MAG_BertForSequenceClassification if kind == "bert" else MAG_XLNetForSequenceClassification
    m = cls(config(kind, hidden, layers), MultimodalConfig(1.0, 0.5), visual_dim=47, acoustic_dim=74)
    return {n: torch.from_numpy(weights.make_param(n, tuple(q.shape), "test")) for n, q in m.named_parameters()}


def build(kind, cdt, hidden=256, layers=LAYERS):
    cls = MAG_BertForSequenceClassification if kind == "bert" else MAG_XLNetForSequenceClassification
    m = cls(config(kind, hidden, layers), MultimodalConfig(1.0, 0.5), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    m.load_state_dict(initial_state(kind, hidden, layers))
    return m


def batch(kind, B, L, seed):
    b = (weights.synthetic_bert_batch if kind == "bert" else weights.synthetic_xlnet_batch)(B, L, 47, 74, seed=seed)
    t = lambda k: torch.from_numpy(b[k]).to(DEV)
    return t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"), t("label_ids")


def trajectory(kind, cdt, mode, hidden=256, shapes=SMALL, nsteps=3, max_grad_norm=None, weight_decay=0.01, break_pair=None,
               clear_marks_before=None, warmup=1.0):
    """nsteps optimizer updates (dropout on, schedule moving) through model.train_step with layer-wise groups (layer_decay 0.9, a head
    learning rate).  mode: False = training_step + optimizer.step(), True = step prologue + replayed graph.  break_pair = (update,
    group, lr): that group's lr is set by hand before that update.  clear_marks_before = update: before that update the engine's map
    is installed again through the C ABI, which clears its marks, behind the model's back.  warmup: the schedule's warm-up steps (1.0: the
    first update runs at lr 0, as in test_param_groups_gpu.py; 0: at the full rates)."""
    torch.manual_seed(77)
    m = build(kind, cdt, hidden).train()
    opt = AdamW(layerwise_lr_groups(m.named_parameters(), LAYERS, LR, layer_decay=DECAY, head_lr=HEAD, weight_decay=weight_decay), lr=LR,
                max_grad_norm=max_grad_norm)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=warmup, num_training_steps=10)
    core = m._core
    updates, clips = [], []
    with m.stream_scope():
        for s in range(nsteps):
            B, L = shapes[s % len(shapes)]
            if break_pair is not None and s == break_pair[0]:
                opt.param_groups[break_pair[1]]["lr"] = break_pair[2]
            if clear_marks_before is not None and s == clear_marks_before:
                import ctypes as C
                bounds, classes = opt.flat_step_args(core)["map"]
                fn = getattr(_lib.lib(), "mb_%s_set_update_map" % kind)
                _lib.check(fn(core.handle, max(classes) + 1, len(classes), (C.c_size_t * len(bounds))(*bounds), (C.c_int * len(classes))(*classes)))
            m.train_step(*batch(kind, B, L, 90 + s), optimizer=opt, graph=mode)          # graph=True raises when the single call is unavailable
            sch.step()
            if mode is not False:
                updates.append(core.update_stats())
            if max_grad_norm is not None:
                clips.append(opt.last_grad_clip)
    stats = core.graph_stats()
    m.eval()
    data = batch(kind, 4, 24, 99)
    with torch.no_grad():
        logits = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].clone()
    torch.cuda.synchronize()
    return dict(p=m.flat_params.clone(), m=core._adam_m.clone(), v=core._adam_v.clone(), g=m.flat_grads.clone(), logits=logits,
                shadow=core.shadow.clone(), stats=stats, updates=updates, clips=clips, model=m, opt=opt)


_REFS = {}


def reference(kind, cdt):
    """three unfused updates at 16 x 256, B = 4, L = 24: computed once, read by several tests, never changed"""
    if (kind, cdt) not in _REFS:
        run = trajectory(kind, cdt, False)
        run.pop("model"); run.pop("opt")
        _REFS[(kind, cdt)] = run
    return _REFS[(kind, cdt)]


def same_bits(run, ref, what):
    for k in ("p", "m", "v", "shadow", "logits"):
        assert torch.equal(run[k], ref[k]), "%s: %s differs, max %.3e" % (what, k, float((run[k].float() - ref[k].float()).abs().max()))
    assert float(run["g"].abs().max()) == 0.0, what


def spans(run, marked):
    """(offset, numel) of the tensors of the optimizer's undecayed (marked = True) or decayed groups"""
    end = run["model"]._core.n_update_end          # (MAG-XLNet's frozen mask_emb lies behind it)
    flat = [getattr(p, "_mb_flat", None) for g in run["opt"].param_groups if (g["weight_decay"] == 0.0) == marked for p in g["params"]]
    return [f[1:3] for f in flat if f is not None and f[1] < end]


def expected_segments(kind):
    return 2 * LAYERS + 5 if kind == "bert" else 3 * LAYERS + 4          # (test_param_groups_paired_cpu.py derives these from the layouts)


@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_paired_step_equals_the_unfused_path_bit_for_bit(kind, cdt, monkeypatch):
    """16 layers x 256, B = 4, L = 24, three updates through the replayed graph: parameters, both moments, the bf16 shadow and the eval
    logits of a fourth batch on the bits of training_step + optimizer.step() of a twin model; one capture, three replays."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ref = reference(kind, cdt)
    run = trajectory(kind, cdt, True)
    assert ref["stats"] == (0, 0) and run["stats"] == (1, 3), (ref["stats"], run["stats"])
    same_bits(run, ref, "%s paired" % kind)
    opt, core = run["opt"], run["model"]._core
    assert len(opt.param_groups) == (36 if kind == "bert" else 35)
    args = opt.flat_step_args(core)
    assert len(args["classes"]["lr"]) == LAYERS + 2 and sum(args["no_decay"]) > 0
    n = core.n_update_end
    for ridden, swept, segs in run["updates"]:
        assert ridden + swept == n and segs == len(args["map"][1]) == expected_segments(kind)


def test_paired_riders_at_768(monkeypatch):
    """MAG-BERT 16 layers x 768, B = 24, L = 50, bf16, where the weight-gradient launches carry riders: ridden slices are clamped to
    their segment and read its slot of the class table.  Riders on, riders off and the unfused path end on the same bits."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    monkeypatch.setenv("MB_GROUP_WGRAD", "256")
    shapes = ((24, 50),)
    monkeypatch.setenv("MB_ADAMW_RIDE", "1")
    ride = trajectory("bert", torch.bfloat16, True, hidden=768, shapes=shapes)
    monkeypatch.setenv("MB_ADAMW_RIDE", "0")
    plain = trajectory("bert", torch.bfloat16, True, hidden=768, shapes=shapes)
    ref = trajectory("bert", torch.bfloat16, False, hidden=768, shapes=shapes)
    same_bits(ride, ref, "paired, riders on")
    same_bits(plain, ref, "paired, riders off")
    n = ride["model"]._core.n_update_end
    ridden, swept, segs = ride["updates"][-1]
    print("paired step at 16 x 768, T = 1200: ridden %d swept %d of %d, %d segments" % (ridden, swept, n, segs))
    assert ridden > 0 and ridden + swept == n and segs == expected_segments("bert")
    assert plain["updates"][-1][:2] == (0, n)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_paired_step_with_gradient_clipping(kind, monkeypatch):
    """max_grad_norm = 0.1 at 16 x 256: the finalize launch multiplies the coefficient into both halves of the class table.  (norm,
    coef) of every update and all state equal the unfused path's, and the gradient really was clipped."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ref = trajectory(kind, torch.bfloat16, False, max_grad_norm=0.1)
    run = trajectory(kind, torch.bfloat16, True, max_grad_norm=0.1)
    print("%s paired + clipping: (norm, coef) fused %s unfused %s" % (kind, run["clips"], ref["clips"]))
    same_bits(run, ref, "%s paired + clipping" % kind)
    assert run["clips"] == ref["clips"] and len(run["clips"]) == 3
    assert all(np.isfinite(nrm) and 0.0 < coef < 1.0 for nrm, coef in run["clips"])
    assert run["stats"] == (1, 3) and all(u[0] == 0 for u in run["updates"])
    assert not torch.equal(run["p"], reference(kind, torch.bfloat16)["p"])          # (clipping changed the trajectory)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_only_unmarked_segments_feel_the_class_weight_decay(kind, monkeypatch):
    """ONE update from one state with weight_decay 0.01 and 0.5 in every decaying group -- the value the paired classes carry.  The
    gradients are the same, so both moments are the same bits everywhere; the tensors of the undecayed groups (marked segments) end on
    the same bits, and every tensor of a decayed group differs -- a mark that decays, or an unmarked segment that does not, shows."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    a = trajectory(kind, torch.bfloat16, True, nsteps=1, weight_decay=0.01, warmup=0)
    b = trajectory(kind, torch.bfloat16, True, nsteps=1, weight_decay=0.5, warmup=0)
    assert a["stats"] == b["stats"] == (1, 1)
    assert "no_decay" in a["opt"].flat_step_args(a["model"]._core)
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"])
    marked, unmarked = spans(a, True), spans(a, False)
    assert len(marked) > LAYERS and len(unmarked) > LAYERS
    for off, numel in marked:
        assert torch.equal(a["p"][off: off + numel], b["p"][off: off + numel]), off
    for off, numel in unmarked:
        assert not torch.equal(a["p"][off: off + numel], b["p"][off: off + numel]), off
    # and against the unfused update with the larger decay, everything
    same_bits(b, trajectory(kind, torch.bfloat16, False, nsteps=1, weight_decay=0.5, warmup=0), "%s weight_decay 0.5" % kind)


def test_a_broken_pair_is_planned_again(monkeypatch):
    """after two updates the undecayed group of layer 3 gets a learning rate of its own: 19 classes, which still fit -- the optimizer
    plans again, the engine gets a map with one mark fewer and captures a second graph, and the third update equals the unfused path's."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    k = 2 * 4 + 1
    ref = trajectory("bert", torch.bfloat16, False, break_pair=(2, k, 7e-4))
    run = trajectory("bert", torch.bfloat16, True, break_pair=(2, k, 7e-4))
    assert run["opt"].param_groups[k]["weight_decay"] == 0.0
    same_bits(run, ref, "broken pair")
    assert not torch.equal(run["p"], reference("bert", torch.bfloat16)["p"])
    args = run["opt"].flat_step_args(run["model"]._core)
    assert len(args["classes"]["lr"]) == LAYERS + 3
    assert run["stats"] == (2, 3)                                                  # planned again: a new map, a second capture
    assert [u[2] for u in run["updates"]] == [expected_segments("bert")] * 3       # the segments are the layout's either way


def test_set_update_map_clears_the_marks(monkeypatch):
    """before the third update the same map is installed again through the C ABI: the marks are gone, the graph is captured anew, and
    that update decays the undecayed groups' tensors -- they leave the unfused path's bits, everything else stays on them."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ref = reference("bert", torch.bfloat16)
    run = trajectory("bert", torch.bfloat16, True, clear_marks_before=2)
    assert run["stats"] == (2, 3)
    assert torch.equal(run["m"], ref["m"]) and torch.equal(run["v"], ref["v"])
    for off, numel in spans(run, False):
        assert torch.equal(run["p"][off: off + numel], ref["p"][off: off + numel]), off
    differ = [not torch.equal(run["p"][off: off + numel], ref["p"][off: off + numel]) for off, numel in spans(run, True)]
    assert all(differ), "%d of %d undecayed tensors kept their bits" % (len(differ) - sum(differ), len(differ))


def test_driver_epoch_with_layerwise_decay_on_a_deep_model(monkeypatch):
    """--model bert-large-uncased --synthetic 96 --n_epochs 1 --layer_lr_decay 0.9 with the model's configuration cut to 16 layers x
    256: a finite loss, and every update went through the single call (one graph launch per step, a map with marks)."""
    from bert_multimodal_transformer_amd import multimodal_driver as D
    monkeypatch.setattr(D, "bert_config", lambda model, num_labels=1: config("bert", 256, LAYERS))
    old = getattr(D, "args", None)
    try:
        D.args = D.parse_args(["--model", "bert-large-uncased", "--synthetic", "96", "--n_epochs", "1", "--layer_lr_decay", "0.9", "--seed", "5"])
        D.set_random_seed(D.args.seed)
        tr, dev, te, nsteps = D.set_up_data_loader()
        m, opt, sch = D.prep_for_training(nsteps)
        assert m.config.num_hidden_layers == LAYERS and len(opt.param_groups) == 36
        loss = D.train_epoch(m, tr, opt, sch)
        torch.cuda.synchronize()
        captures, launches = m._core.graph_stats()
        ridden, swept, segs = m._core.update_stats()
        print("driver, 16 x 256 layer-wise: train loss %.4f, %d steps, %d graph launches, %d segments" % (loss, len(tr), launches, segs))
        assert np.isfinite(loss) and launches == len(tr) == opt._t > 0
        assert segs == expected_segments("bert") and "no_decay" in opt.flat_step_args(m._core)
    finally:
        D.args = old
