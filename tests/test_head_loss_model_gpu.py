"""Head losses through the models: both engines, 2 layers, B = 6, L = 32, dropout 0.

Pattern and bounds are those of test_fused_cross_entropy_step_num_labels_3 (tests/test_model_gpu.py): the fused step's loss within
2e-5 * max(1, |loss|) and every parameter gradient within 5e-3 of max(|g|, 1e-3 g_max) of the ORACLE model's logits put through
torch's own loss function and autograd on the CPU; the autograd route, the single-call step (graph) and the stage-driven step within
1e-5 * max|g| + 1e-9 of the fused gradients.  bf16: twice the worst relative gradient error of the default loss on the same bf16 model
and batch, measured in the same test (MB_HEAD_LOSS_REPORT=<file> appends the figures: profiles/head_loss_errors.txt)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, BertConfig, MAG_BertForSequenceClassification, MAG_XLNetForSequenceClassification,
                                             MultimodalConfig, XLNetConfig)
from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
from oracle import mag_bert_ref as R
from oracle import mag_xlnet_ref as X
from oracle import weights

DEV = "cuda:0"
F = torch.nn.functional
LAYERS, B, L = 2, 6, 32
PW = (0.5, 1.0, 3.0)            # bce's pos_weight: below, at and above 1
CW = (0.0, 1.5, 0.5)            # class weights with a zero
# (label, set_loss arguments, num_labels)
CASES = [("mse", dict(name="mse"), 1), ("l1", dict(name="l1"), 1), ("smooth_l1", dict(name="smooth_l1", beta=1.0), 1),
         ("default", dict(name="default"), 3), ("mse", dict(name="mse"), 3), ("l1", dict(name="l1"), 3),
         ("smooth_l1", dict(name="smooth_l1", beta=0.5), 3), ("bce", dict(name="bce"), 3), ("bce pos_weight", dict(name="bce", pos_weight=PW), 3),
         ("cross_entropy", dict(name="cross_entropy"), 3), ("cross_entropy weight", dict(name="cross_entropy", weight=CW), 3)]
_PAIRS = {}


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


def build(kind, nl, cdt=torch.float32):
    if kind == "bert":
        cfg = BertConfig(num_hidden_layers=LAYERS, num_labels=nl, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        m = MAG_BertForSequenceClassification(cfg, MultimodalConfig(1.0, 0.0), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    else:
        m = MAG_XLNetForSequenceClassification(XLNetConfig(n_layer=LAYERS, num_labels=nl, dropout=0.0, summary_last_dropout=0.0),
                                               MultimodalConfig(1.0, 0.0), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    m.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(p.shape), "test")) for n, p in m.named_parameters()})
    return m.train()


def build_oracle(kind, nl):
    if kind == "bert":
        o = R.MAG_BertForSequenceClassification(R.BertConfigLite(num_hidden_layers=LAYERS, num_labels=nl), R.MultimodalConfig(1.0, 0.0), 47, 74)
        o = R.set_dropout(o, 0.0, 0.0, 0.0)
    else:
        o = X.set_dropout(X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(n_layer=LAYERS, num_labels=nl), X.MultimodalConfig(1.0, 0.0), 47, 74), 0.0, 0.0)
    names = dict(o.named_parameters())
    o.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(p.shape), "test")) for n, p in names.items()}, strict=False)
    return o.train()


def batch(kind, dev="cpu", seed=61):
    b = (weights.synthetic_bert_batch if kind == "bert" else weights.synthetic_xlnet_batch)(B, L, 47, 74, seed=seed)
    t = lambda k: torch.from_numpy(b[k]).to(dev)
    return t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids")


def torch_loss(args, logits, y):
    """torch's own function of that name on [B, nl] logits"""
    name = args["name"]
    nl = logits.shape[1]
    vec = lambda v: None if v is None else torch.tensor(v, dtype=logits.dtype)
    if name == "default":
        return F.mse_loss(logits.view(-1), y.view(-1)) if nl == 1 else F.cross_entropy(logits, y.long())
    if name == "cross_entropy":
        return F.cross_entropy(logits, y.long(), weight=vec(args.get("weight")))
    y = y.view(-1, nl)
    if name == "mse":
        return F.mse_loss(logits, y)
    if name == "l1":
        return F.l1_loss(logits, y)
    if name == "smooth_l1":
        return F.smooth_l1_loss(logits, y, beta=args["beta"])
    return F.binary_cross_entropy_with_logits(logits, y, pos_weight=vec(args.get("pos_weight")))


def random_targets(args, nl, seed=5):
    g = torch.Generator().manual_seed(seed)
    name = args["name"]
    if name == "cross_entropy" or (name == "default" and nl > 1):
        return torch.tensor([0, 2, 1, 1, 0, 2])
    if name == "default":
        return torch.randn(B, generator=g)
    if name == "bce":
        y = torch.rand(B, nl, generator=g)
        y[0, 0], y[1, -1], y[2, 0] = 0.0, 1.0, 0.5
        return y
    return torch.randn(B, nl, generator=g)


def oracle_grads(o, kind, args, y):
    o.zero_grad()
    logits = o(*batch(kind))[0]
    loss = torch_loss(args, logits.view(B, -1), y)
    loss.backward()
    return float(loss.detach()), {n: p.grad.clone() for n, p in o.named_parameters() if p.grad is not None}, logits.detach().view(B, -1)


def worst_rel(m, og):
    gmax = max(float(g.abs().max()) for g in og.values())
    return max((float((p.grad.cpu().float() - og[n]).abs().max()) / max(float(og[n].abs().max()), 1e-3 * gmax), n)
               for n, p in m.named_parameters() if n in og)


def report(line):
    print(line)
    path = os.environ.get("MB_HEAD_LOSS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("label,args,nl", CASES, ids=["%s-nl%d" % (c[0].replace(" ", "_"), c[2]) for c in CASES])
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_every_route_runs_the_configured_loss(kind, label, args, nl):
    m, o = pair(kind, nl)
    m.set_loss(**args)
    assert m.loss.name == args["name"] and m.loss.beta == args.get("beta") and m.loss.vector == (args.get("pos_weight") or args.get("weight"))
    y = random_targets(args, nl)
    lo, og, _ = oracle_grads(o, kind, args, y)
    ids, vis, aco, mask, seg = batch(kind, DEV)
    yd = y.to(DEV)
    l_fused = m.training_step(ids, vis, aco, mask, seg, yd)
    torch.cuda.synchronize()
    worst = worst_rel(m, og)
    print("%s %s nl=%d: loss %.6f (oracle %.6f), worst relative gradient error %.2e at %s" % (kind, label, nl, float(l_fused), lo, worst[0], worst[1]))
    assert abs(float(l_fused) - lo) <= 2e-5 * max(1.0, abs(lo)), (float(l_fused), lo)
    assert worst[0] <= 5e-3, worst
    g_fused = m.flat_grads.clone()
    bound = 1e-5 * float(g_fused.abs().max()) + 1e-9
    m.zero_grad()
    out = m(ids, vis, aco, attention_mask=mask, token_type_ids=seg, labels=yd)                   # the autograd route
    out[0].backward()
    assert abs(float(out[0]) - lo) <= 2e-5 * max(1.0, abs(lo))
    assert float((m.flat_grads - g_fused).abs().max()) <= bound, "autograd route"
    m.zero_grad()
    l_graph = m.train_step(ids, vis, aco, mask, seg, yd, optimizer=None)                           # the single-call step: a graph
    torch.cuda.synchronize()
    assert abs(float(l_graph) - lo) <= 2e-5 * max(1.0, abs(lo))
    assert float((m.flat_grads - g_fused).abs().max()) <= bound, "single-call step"
    if kind == "bert":                                                                              # (the stage-driven passes are MAG-BERT's)
        m.zero_grad()
        m._core.stage_step(ids, vis, aco, mask, seg, yd)
        torch.cuda.synchronize()
        assert abs(float(m._core.loss_buf[0]) - lo) <= 2e-5 * max(1.0, abs(lo))
        assert float((m.flat_grads - g_fused).abs().max()) <= bound, "stage-driven step"
    # eval_step accumulates the configured loss into the running sum
    m.eval()
    m.loss_running(reset=True)
    with torch.no_grad():
        m.eval_step(ids, vis, aco, mask, seg, yd)
        m.eval_step(ids, vis, aco, mask, seg, yd)
    assert abs(float(m.loss_running(reset=True)) - 2 * lo) <= 4e-5 * max(1.0, abs(lo))
    m.train()
    m.set_loss("default")


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_switching_the_loss_between_steps(kind, monkeypatch):
    """mse, l1, mse again on one model through the graph: the setter drops the captured step, so the step after it runs the new loss,
    and the step after setting the old one back runs the old one -- bit for bit (deterministic sums: MB_DETERMINISTIC=1)"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    m, fresh = build(kind, 1), build(kind, 1)
    ids, vis, aco, mask, seg = batch(kind, DEV)
    y = torch.randn(B, 1, generator=torch.Generator().manual_seed(8)).to(DEV)
    grads = []
    for name in ("mse", "l1", "mse"):
        m.set_loss(name)
        m.zero_grad()
        m.train_step(ids, vis, aco, mask, seg, y, optimizer=None, graph=True)
        torch.cuda.synchronize()
        grads.append(m.flat_grads.clone())
    assert torch.equal(grads[0], grads[2]) and not torch.equal(grads[0], grads[1])
    assert m._core.graph_stats() == (3, 3)                                   # every change captured anew
    fresh.set_loss("l1")
    fresh.train_step(ids, vis, aco, mask, seg, y, optimizer=None, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(fresh.flat_grads, grads[1])
    # the default kind at one label is mse: the same bits, and setting what is set drops nothing
    m.set_loss("mse")
    m.set_loss("default")
    m.zero_grad()
    m.train_step(ids, vis, aco, mask, seg, y.view(-1), optimizer=None, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(m.flat_grads, grads[0]) and m._core.graph_stats() == (4, 4)


@pytest.mark.parametrize("kind,args,nl", [("bert", dict(name="l1"), 1), ("xlnet", dict(name="bce", pos_weight=PW), 3)])
def test_single_call_step_with_optimizer_equals_the_unfused_path(kind, args, nl, monkeypatch):
    """two train_step calls (graph) end on the bits of training_step() + optimizer.step(), as tests/test_param_groups_gpu.py asserts for
    the default loss"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ends = []
    for graph in (False, True):
        m = build(kind, nl)
        m.set_loss(**args)
        opt = AdamW(optimizer_grouped_parameters(m), lr=1e-3)
        with m.stream_scope():
            for s in range(2):
                ids, vis, aco, mask, seg = batch(kind, DEV, seed=70 + s)
                y = random_targets(args, nl, seed=s).to(DEV)
                m.train_step(ids, vis, aco, mask, seg, y, optimizer=opt, graph=graph)
        torch.cuda.synchronize()
        ends.append((m.flat_params.clone(), m._core._adam_m.clone(), m._core._adam_v.clone(), m._core.graph_stats()))
    assert ends[0][3] == (0, 0) and ends[1][3][0] >= 1 and ends[1][3][1] == 2, (ends[0][3], ends[1][3])       # no graph | two replays
    for a, b, what in zip(ends[0][:3], ends[1][:3], ("parameters", "m", "v")):
        assert torch.equal(a, b), "%s differ, max %.3e" % (what, float((a - b).abs().max()))


BF16_CASES = [("mse", dict(name="mse"), 1), ("l1", dict(name="l1"), 1), ("smooth_l1", dict(name="smooth_l1", beta=1.0), 1),
              ("bce", dict(name="bce", pos_weight=PW), 3), ("cross_entropy", dict(name="cross_entropy", weight=CW), 3)]


def bf16_targets(args, logits, nl):
    """targets from the oracle's own logits, so that no sample sits near a kink (bf16 logits lie within 1.1e-2 of fp32)"""
    name = args["name"]
    sign = torch.tensor([1.0, -1.0] * (B // 2)).view(B, 1)
    if name == "l1":
        delta = torch.tensor([0.25, 0.5, 1.0, 0.3, 2.0, 0.75]).view(B, 1)              # y = logit +- delta, delta >= 0.25
        return logits + sign * delta
    if name == "smooth_l1":
        delta = torch.tensor([0.5, 0.1, 0.3, 2.0, 3.0, 2.5]).view(B, 1)                # half inside beta = 1 (<= 0.5), half outside (>= 2)
        return logits + sign * delta
    return random_targets(args, nl)


@pytest.mark.parametrize("label,args,nl", BF16_CASES, ids=[c[0] for c in BF16_CASES])
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_bf16(kind, label, args, nl):
    m, o = pair(kind, nl, torch.bfloat16)
    ids, vis, aco, mask, seg = batch(kind, DEV)
    # the yardstick: the default loss on this model and batch against this oracle
    dflt = dict(name="default")
    y0 = random_targets(dflt, nl)
    _, og0, logits = oracle_grads(o, kind, dflt, y0)
    m.set_loss("default")
    m.training_step(ids, vis, aco, mask, seg, y0.to(DEV))
    torch.cuda.synchronize()
    base = worst_rel(m, og0)
    y = bf16_targets(args, logits, nl)
    lo, og, _ = oracle_grads(o, kind, args, y)
    m.zero_grad()
    m.set_loss(**args)
    l_fused = m.training_step(ids, vis, aco, mask, seg, y.to(DEV))
    torch.cuda.synchronize()
    worst = worst_rel(m, og)
    m.set_loss("default")
    report("bf16 %-5s %-14s nl=%d: loss %.6f (oracle %.6f), worst relative gradient error %.3e at %s; default loss on the same model and batch "
           "%.3e at %s; bound %.3e" % (kind, label, nl, float(l_fused), lo, worst[0], worst[1], base[0], base[1], 2 * base[0]))
    assert worst[0] <= 2 * base[0], (worst, base)


def test_driver_with_l1(capsys, monkeypatch):
    """main() with --loss l1: eval_epoch's value is the mean absolute error of test_epoch's predictions on the same split"""
    from bert_multimodal_transformer_amd import multimodal_driver as D
    seen = {}
    train = D.train

    def keep(model, train_loader, dev_loader, test_loader, optimizer, scheduler):
        seen.update(model=model, dev=dev_loader, opt=optimizer)
        return train(model, train_loader, dev_loader, test_loader, optimizer, scheduler)

    monkeypatch.setattr(D, "train", keep)
    D.main(["--synthetic", "96", "--n_epochs", "1", "--loss", "l1", "--train_batch_size", "24"])
    out = capsys.readouterr().out
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert len(recs) == 1 and all(np.isfinite(recs[0][k]) for k in ("train_loss", "valid_loss", "test_mae"))
    model = seen["model"]
    assert model.loss.name == "l1"
    value = D.eval_epoch(model, seen["dev"], seen["opt"])
    preds, labels = D.test_epoch(model, seen["dev"])
    assert len(seen["dev"]) == 1                                             # (one batch: the mean over batches is the mean over samples)
    mae = float(np.abs(preds.astype(np.float64) - labels).mean())
    assert abs(value - mae) <= 1e-5, (value, mae)
    assert abs(recs[0]["valid_loss"] - mae) <= 1e-5
    # the options default to the reference's objective, and refuse what the driver does not train
    assert D.parse_args(["--synthetic", "8"]).loss is None and D.parse_args(["--loss", "smooth_l1", "--loss_beta", "0.5"]).loss_beta == 0.5
    with pytest.raises(SystemExit):
        D.parse_args(["--loss", "bce"])
