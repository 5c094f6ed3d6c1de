"""The head-loss options through the models: both engines, 2 layers x 256, B = 5, L = 8, dropout 0; num_labels = 5 for the cross entropy,
3 for bce.  The ORACLE model's logits are put through losses.torch_loss in float64 (the objective's host statement, pinned against
torch.nn.functional and the fp64 formulas by tests/test_head_loss_options_cpu.py) and compared with training_step, train_step with and
without the graph, eval_step and forward(labels=...).

Bounds: those tests/test_head_loss_model_gpu.py uses for the weighted cross entropy.  fp32 (its lines 146-159, the pattern of
test_fused_cross_entropy_step_num_labels_3): the loss within 2e-5 * max(1, |loss|) and every parameter gradient within 5e-3 of
max(|g|, 1e-3 g_max) of the oracle's; every other route within 1e-5 * max|g| + 1e-9 of the fused gradients.  bf16 (its line 269): the
worst relative gradient error at most twice that of the default loss on the same bf16 model and batch, measured in the same test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, BertConfig, MAG_BertForSequenceClassification, MAG_XLNetForSequenceClassification,
                                             MultimodalConfig, XLNetConfig, losses)
from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
from oracle import mag_bert_ref as R
from oracle import mag_xlnet_ref as X
from oracle import weights

DEV = "cuda:0"
LAYERS, H, HEADS, INNER, B, L = 2, 256, 4, 1024, 5, 8
CW = (0.0, 1.5, 0.5, 1.0, 2.0)          # class weights with a zero
PW = (0.5, 1.0, 3.0)                    # bce's pos_weight: below, at and above 1
# (label, set_loss arguments, num_labels, labels)
CASES = [("ce eps=0.1 weight ignore", dict(name="cross_entropy", label_smoothing=0.1, weight=CW, ignore_index=-100), 5,
          torch.tensor([4, -100, 1, -100, 2])),                                              # two ignored samples
         ("ce gamma=2", dict(name="cross_entropy", focal_gamma=2.0), 5, torch.tensor([4, 0, 1, 3, 2])),
         ("bce gamma=2 pos_weight", dict(name="bce", focal_gamma=2.0, pos_weight=PW), 3,
          torch.tensor([[0.0, 1.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.5, 0.0, 1.0]]))]
IDS = [c[0].replace(" ", "_") for c in CASES]
_PAIRS = {}


def build(kind, nl, cdt=torch.float32):
    if kind == "bert":
        cfg = BertConfig(hidden_size=H, num_attention_heads=HEADS, intermediate_size=INNER, num_hidden_layers=LAYERS, num_labels=nl,
                         hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        m = MAG_BertForSequenceClassification(cfg, MultimodalConfig(1.0, 0.0), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    else:
        cfg = XLNetConfig(d_model=H, n_head=HEADS, d_inner=INNER, n_layer=LAYERS, num_labels=nl, dropout=0.0, summary_last_dropout=0.0)
        m = MAG_XLNetForSequenceClassification(cfg, MultimodalConfig(1.0, 0.0), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    m.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(p.shape), "test")) for n, p in m.named_parameters()})
    return m.train()


def build_oracle(kind, nl):
    if kind == "bert":
        o = R.MAG_BertForSequenceClassification(R.BertConfigLite(hidden_size=H, num_attention_heads=HEADS, intermediate_size=INNER,
                                                                 num_hidden_layers=LAYERS, num_labels=nl), R.MultimodalConfig(1.0, 0.0), 47, 74)
        o = R.set_dropout(o, 0.0, 0.0, 0.0)
    else:
        o = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(d_model=H, n_head=HEADS, d_inner=INNER, n_layer=LAYERS, num_labels=nl),
                                                 X.MultimodalConfig(1.0, 0.0), 47, 74)
        o = X.set_dropout(o, 0.0, 0.0)
    o.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(p.shape), "test")) for n, p in o.named_parameters()}, strict=False)
    return o.train()


def pair(kind, nl, cdt=torch.float32):
    """(model, oracle) with the same weights; built once per (model kind, num_labels, dtype) -- the tests switch its loss"""
    key = (kind, nl, cdt)
    if key not in _PAIRS:
        _PAIRS[key] = (build(kind, nl, cdt), build_oracle(kind, nl))
    m, o = _PAIRS[key]
    m.train()
    m.zero_grad()
    o.zero_grad()
    return m, o


def batch(kind, dev="cpu", seed=61):
    b = (weights.synthetic_bert_batch if kind == "bert" else weights.synthetic_xlnet_batch)(B, L, 47, 74, seed=seed)
    t = lambda k: torch.from_numpy(b[k]).to(dev)
    return t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids")


def oracle_grads(o, kind, loss, y, nl):
    """the oracle's logits through losses.torch_loss in float64, and autograd from there"""
    o.zero_grad()
    logits = o(*batch(kind))[0]
    value = losses.torch_loss(loss, logits.view(B, nl).double(), y, nl)
    value.backward()
    return float(value.detach()), {n: p.grad.clone() for n, p in o.named_parameters() if p.grad is not None}


def worst_rel(m, og):
    gmax = max(float(g.abs().max()) for g in og.values())
    return max((float((p.grad.cpu().float() - og[n]).abs().max()) / max(float(og[n].abs().max()), 1e-3 * gmax), n)
               for n, p in m.named_parameters() if n in og)


@pytest.mark.parametrize("label,args,nl,y", CASES, ids=IDS)
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_every_route_runs_the_configured_objective(kind, label, args, nl, y):
    m, o = pair(kind, nl)
    m.set_loss(**args)
    assert m.loss == losses.make_loss(args["name"], nl, **{k: v for k, v in args.items() if k != "name"})
    lo, og = oracle_grads(o, kind, m.loss, y, nl)
    ids, vis, aco, mask, seg = batch(kind, DEV)
    yd = y.to(DEV)
    near = lambda v: abs(float(v) - lo) <= 2e-5 * max(1.0, abs(lo))
    l_fused = m.training_step(ids, vis, aco, mask, seg, yd)
    torch.cuda.synchronize()
    worst = worst_rel(m, og)
    print("%s %s: loss %.6f (oracle %.6f), worst relative gradient error %.2e at %s" % (kind, label, float(l_fused), lo, worst[0], worst[1]))
    assert near(l_fused), (float(l_fused), lo)
    assert worst[0] <= 5e-3, worst
    g_fused = m.flat_grads.clone()
    bound = 1e-5 * float(g_fused.abs().max()) + 1e-9
    for graph in (True, False):                                                                       # the single-call step
        m.zero_grad()
        l_step = m.train_step(ids, vis, aco, mask, seg, yd, optimizer=None, graph=graph)
        torch.cuda.synchronize()
        assert near(l_step), (graph, float(l_step), lo)
        assert float((m.flat_grads - g_fused).abs().max()) <= bound, "train_step graph=%s" % graph
    m.zero_grad()
    out = m(ids, vis, aco, attention_mask=mask, token_type_ids=seg, labels=yd)                        # the autograd route
    out[0].backward()
    assert near(out[0]), (float(out[0]), lo)
    assert float((m.flat_grads - g_fused).abs().max()) <= bound, "autograd route"
    m.eval()                                                                                          # eval_step: the running sum
    m.loss_running(reset=True)
    with torch.no_grad():
        m.eval_step(ids, vis, aco, mask, seg, yd)
        m.eval_step(ids, vis, aco, mask, seg, yd)
    assert abs(float(m.loss_running(reset=True)) - 2 * lo) <= 4e-5 * max(1.0, abs(lo))
    m.train()
    m.set_loss("default")


@pytest.mark.parametrize("label,args,nl,y", CASES, ids=IDS)
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_bf16(kind, label, args, nl, y):
    m, o = pair(kind, nl, torch.bfloat16)
    ids, vis, aco, mask, seg = batch(kind, DEV)
    # the yardstick: the default loss on this model and batch against this oracle
    y0 = torch.tensor([4, 0, 1, 3, 2]) % nl
    m.set_loss("default")
    _, og0 = oracle_grads(o, kind, m.loss, y0, nl)
    m.training_step(ids, vis, aco, mask, seg, y0.to(DEV))
    torch.cuda.synchronize()
    base = worst_rel(m, og0)
    m.zero_grad()
    m.set_loss(**args)
    lo, og = oracle_grads(o, kind, m.loss, y, nl)
    l_fused = m.training_step(ids, vis, aco, mask, seg, y.to(DEV))
    torch.cuda.synchronize()
    worst = worst_rel(m, og)
    m.set_loss("default")
    print("bf16 %-5s %-26s: loss %.6f (oracle %.6f), worst relative gradient error %.3e at %s; default loss %.3e at %s; bound %.3e"
          % (kind, label, float(l_fused), lo, worst[0], worst[1], base[0], base[1], 2 * base[0]))
    assert worst[0] <= 2 * base[0], (worst, base)


@pytest.mark.parametrize("kind,case", [("bert", 0), ("xlnet", 2)])
def test_single_call_step_with_optimizer_equals_the_unfused_path(kind, case, monkeypatch):
    """deterministic sums: two train_step calls through the graph end on the bits of training_step() + optimizer.step() (graph=False)"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    _, args, nl, y = CASES[case]
    ends = []
    for graph in (False, True):
        m = build(kind, nl)
        m.set_loss(**args)
        opt = AdamW(optimizer_grouped_parameters(m), lr=1e-3)
        with m.stream_scope():
            for s in range(2):
                ids, vis, aco, mask, seg = batch(kind, DEV, seed=70 + s)
                m.train_step(ids, vis, aco, mask, seg, y.to(DEV), optimizer=opt, graph=graph)
        torch.cuda.synchronize()
        ends.append((m.flat_params.clone(), m._core._adam_m.clone(), m._core._adam_v.clone(), m._core.graph_stats()))
    assert ends[0][3] == (0, 0) and ends[1][3][0] >= 1 and ends[1][3][1] == 2, (ends[0][3], ends[1][3])       # no graph | two replays
    for a, b, what in zip(ends[0][:3], ends[1][:3], ("parameters", "m", "v")):
        assert torch.equal(a, b), "%s differ, max %.3e" % (what, float((a - b).abs().max()))
        assert bool(torch.isfinite(a).all()), what


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_changing_an_option_between_graph_steps(kind, monkeypatch):
    """smoothing, then gamma, then an ignored sample, on one model through the graph: every change drops the captured step, the step
    after it runs the new objective -- its loss and gradients are those of graph=False on a fresh model"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    m, fresh = build(kind, 5), build(kind, 5)
    ids, vis, aco, mask, seg = batch(kind, DEV)
    y = torch.tensor([4, 0, 1, 3, 2]).to(DEV)
    yi = torch.tensor([4, -100, 1, 3, 2]).to(DEV)
    seen = []
    for n, (kw, yy) in enumerate(((dict(label_smoothing=0.1), y), (dict(focal_gamma=2.0), y), (dict(focal_gamma=2.0, ignore_index=-100), yi),
                                  (dict(), y))):
        for mm, graph in ((m, True), (fresh, False)):
            mm.set_loss("cross_entropy", **kw)
            mm.zero_grad()
            loss = mm.train_step(ids, vis, aco, mask, seg, yy, optimizer=None, graph=graph)
            torch.cuda.synchronize()
            seen.append((float(loss), mm.flat_grads.clone()))
        assert seen[-2][0] == seen[-1][0] and torch.equal(seen[-2][1], seen[-1][1]), (n, kw, seen[-2][0], seen[-1][0])
        assert m._core.graph_stats() == (n + 1, n + 1)                       # every change captured anew
    assert len({s[0] for s in seen}) == 4                                    # four objectives, four losses
    m.set_loss("cross_entropy")                                              # setting what is set drops nothing
    m.zero_grad()                                                            # (a cleared gradient buffer is part of the graph's identity)
    m.train_step(ids, vis, aco, mask, seg, y, optimizer=None, graph=True)
    assert m._core.graph_stats() == (4, 5)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_an_all_ignored_batch_is_refused_on_the_host(kind):
    m, _ = pair(kind, 5)
    m.set_loss("cross_entropy", ignore_index=-100)
    ids, vis, aco, mask, seg = batch(kind, DEV)
    y = torch.full((B,), -100).to(DEV)
    before = m._core.graph_stats()
    for call in (lambda: m.training_step(ids, vis, aco, mask, seg, y), lambda: m.train_step(ids, vis, aco, mask, seg, y, optimizer=None, graph=True),
                 lambda: m.eval_step(ids, vis, aco, mask, seg, y)):
        with pytest.raises(ValueError, match="every label"):
            call()
    assert m._core.graph_stats() == before                                   # (the check sits in _inputs, in front of every enqueue)
    m.set_loss("default")
