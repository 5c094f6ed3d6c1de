"""GPU: frozen embeddings and encoder layers in the single-call training step.

"Frozen" = in no parameter group of the optimizer (model.freeze sets requires_grad, the group builders leave such parameters out).
The yardstick is the path that has always handled a partly covered buffer: train_step(..., graph=False) = training_step() +
optimizer.step() over the covered ranges, with full compute.  In deterministic mode the single-call step -- which leaves out the
weight-gradient launches of frozen layers and the embedding backward -- ends every trainable tensor on its bits, keeps the frozen
parameters and their shadow, leaves their moments exactly zero and the whole gradient buffer zero.  The oracle cases compare with
oracle.optim_ref.AdamW over the oracle model with the same tensors left out."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, BertConfig, MAG_BertForSequenceClassification, MAG_XLNetForSequenceClassification,
                                             MultimodalConfig, XLNetConfig, get_linear_schedule_with_warmup, layerwise_lr_groups, _lib)
from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
from oracle import mag_bert_ref as R
from oracle import mag_xlnet_ref as X
from oracle import optim_ref as O
from oracle import weights

DEV = "cuda:0"
LR, DECAY, HEAD = 1e-3, 0.5, 5e-3
SMALL = ((5, 40), (5, 40), (3, 24), (5, 40))
BIG = ((24, 50), (24, 50), (5, 40), (24, 50))          # T = 1200: every rider host carries
EMB_LOW2 = (True, (0, 1))                               # embeddings + layers 0 - 1 of 3


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(kind, layers, cdt, dropout=True):
    p, pm = (0.1, 0.5) if dropout else (0.0, 0.0)
    if kind == "bert":
        cfg = BertConfig(num_hidden_layers=layers, num_labels=1, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
        m = MAG_BertForSequenceClassification(cfg, MultimodalConfig(1.0, pm), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    else:
        cfg = XLNetConfig(n_layer=layers, num_labels=1, dropout=p, summary_last_dropout=p)
        m = MAG_XLNetForSequenceClassification(cfg, MultimodalConfig(1.0, pm), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    m.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(q.shape), "test")) for n, q in m.named_parameters()})
    return m


def batch(kind, B, L, seed, dev=DEV, label_mult=1.0):
    b = (weights.synthetic_bert_batch if kind == "bert" else weights.synthetic_xlnet_batch)(B, L, 47, 74, seed=seed)
    t = lambda k: torch.from_numpy(b[k]).to(dev)
    return t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"), t("label_ids") * label_mult


def apply_freeze(m, freeze):
    """freeze: (embeddings, layers) for model.freeze, or a tuple of name fragments frozen by hand (a partial layer)"""
    if freeze is None:
        return []
    if isinstance(freeze[0], str):
        names = [n for n, _ in m.named_parameters() if any(f in n for f in freeze)]
        for n, p in m.named_parameters():
            if n in names:
                p.requires_grad_(False)
        return names
    return m.freeze(embeddings=freeze[0], layers=freeze[1])


def make_groups(m, groups, layers):
    if groups == "classed":
        return layerwise_lr_groups(m.named_parameters(), layers, LR, layer_decay=DECAY, head_lr=HEAD)
    return optimizer_grouped_parameters(m)


def frozen_mask(m, names):
    mask = torch.zeros(m._core.n_params, dtype=torch.bool, device=DEV)
    by_name = dict(m.named_parameters())
    for n in names:
        info = getattr(by_name[n], "_mb_flat", None)
        if info is not None:
            mask[info[1]: (info[1] + info[2] + 63) // 64 * 64] = True
    return mask


@functools.lru_cache(maxsize=None)
def trajectory(kind, cdt, mode, freeze=EMB_LOW2, groups="driver", shapes=SMALL, nsteps=4, accum=1, layers=3, max_norm=None, thaw_at=None,
               by_hand=False, envs=()):
    """nsteps optimizer updates (dropout on, schedule moving) through model.train_step, in deterministic mode.  mode: False =
    training_step + optimizer.step(), True = step prologue + replayed graph, 2 = prologue + the same kernels launched one by one.
    thaw_at: before that update the model is unfrozen and a new optimizer (and schedule) over every parameter takes over.  by_hand
    (mode False): the fp64 norm of the trainable `.grad` tensors is read in front of every update.  Returns tensors and records only."""
    with env(MB_DETERMINISTIC=1, **dict(envs)):
        torch.manual_seed(77)
        m = build(kind, layers, cdt).train()
        names = apply_freeze(m, freeze)
        opt = AdamW(make_groups(m, groups, layers), lr=LR, max_grad_norm=max_norm)
        sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
        core = m._core
        start = m.flat_params.clone()
        mask = frozen_mask(m, names)
        upd, frz, gmax, clip, norm64, gfrozen = [], [], [], [], [], []
        with m.stream_scope():
            for s in range(nsteps * accum):
                B, L = shapes[s % len(shapes)]
                u = s // accum
                data = batch(kind, B, L, 90 + s, label_mult=8.0 if (max_norm is not None or by_hand) and u % 2 == 1 else 1.0)
                update = (s + 1) % accum == 0
                if thaw_at is not None and s == thaw_at * accum:
                    m.unfreeze()
                    opt = AdamW(make_groups(m, groups, layers), lr=LR, max_grad_norm=max_norm)
                    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
                if mode == 2:
                    o = opt.flat_step_args(core) if update else None
                    if update:
                        opt._t += 1
                        o["t"] = opt._t
                    core.train_step(*data, o, loss_scale=1.0 / accum, mode=2)
                    if update and o.get("max_grad_norm"):
                        opt._clip_last = core
                elif mode is False and by_hand:
                    m.training_step(*data, loss_scale=1.0 / accum)
                    if update:
                        m.materialize_grads()
                        tot = torch.zeros((), dtype=torch.float64, device=DEV)
                        for _, p in m.named_parameters():
                            if p.grad is not None and p.requires_grad:
                                tot += p.grad.detach().double().pow(2).sum()
                        norm64.append(float(tot.sqrt()))
                        opt.step()
                        opt.zero_grad()
                else:
                    m.train_step(*data, optimizer=opt if update else None, loss_scale=1.0 / accum, graph=mode)
                if update:
                    sch.step()
                    if opt.max_grad_norm:
                        clip.append(opt.last_grad_clip)
                    if mode is not False:
                        upd.append(core.update_stats())
                        frz.append(core.freeze_stats())
                        g = m.flat_grads
                        gmax.append(float(g.abs().max()))
                        gfrozen.append(float(g[mask].abs().max()) if bool(mask.any()) else 0.0)
        stats = core.graph_stats()
        m.eval()
        data = batch(kind, 4, 40, 99)
        with torch.no_grad():
            logits = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].clone()
        torch.cuda.synchronize()
        return dict(p=m.flat_params.clone(), m=core._adam_m.clone(), v=core._adam_v.clone(), logits=logits, shadow=core.shadow.clone(),
                    stats=stats, update=upd, frozen=frz, gmax=gmax, gfrozen=gfrozen, clip=clip, norm64=norm64, start=start,
                    mask=mask, n=core.n_update_end, sh=(core.sh_begin, core.sh_end), names=tuple(names),
                    marks=bool(opt.flat_step_args(core) and opt.flat_step_args(core).get("frozen")))


def same_bits(run, ref, what):
    for k in ("p", "m", "v", "shadow", "logits"):
        assert torch.equal(run[k], ref[k]), "%s: %s differs, max %.3e" % (what, k, float((run[k].float() - ref[k].float()).abs().max()))


def frozen_untouched(run, what):
    """frozen parameters and their shadow on the start's bits, frozen moments exactly zero, the gradient buffer zero after every update"""
    mask = run["mask"]
    assert bool(mask.any()), what
    assert torch.equal(run["p"][mask], run["start"][mask]), what
    if run["shadow"].numel() > 1:          # (fp32 runs keep no bf16 shadow)
        b, e = run["sh"]
        assert torch.equal(run["shadow"][b:e][mask[b:e]], run["start"][b:e][mask[b:e]].to(torch.bfloat16)), what          # (filled by the first forward)
    assert float(run["m"][mask].abs().max()) == 0.0 and float(run["v"][mask].abs().max()) == 0.0, what
    assert not torch.equal(run["p"][~mask], run["start"][~mask]), what
    if run["gmax"]:
        assert max(run["gmax"]) == 0.0 and max(run["gfrozen"]) == 0.0, (what, run["gmax"])


def accounted(run):
    for (ridden, swept, _), (elems, _, _) in zip(run["update"], run["frozen"]):
        assert ridden + swept + elems == run["n"], (ridden, swept, elems, run["n"])


# --------------------------------------------------------------------------------------------- 1 / 2: embeddings + the lower layers
@pytest.mark.parametrize("kind,cdt,groups", [("bert", torch.bfloat16, "driver"), ("bert", torch.float32, "driver"), ("xlnet", torch.bfloat16, "driver"),
                                             ("bert", torch.bfloat16, "classed"), ("xlnet", torch.bfloat16, "classed")])
def test_frozen_embeddings_and_lower_layers(kind, cdt, groups):
    """embeddings + layers 0 - 1 of 3 frozen, the driver's two groups (a two-class map with marks) or layer-wise groups after
    model.freeze (marks and classes together): the replayed graph, the prologue + eager launches and graph=False end p, m, v, the shadow
    and the eval logits of a fifth batch on the same bits; frozen parameters keep the start's bits, their moments are exactly zero,
    the gradient buffer reads zero after every single-call update; two weight-gradient launches and the embedding backward (MAG-XLNet:
    the word scatter) are left out of every step.  Without the feature graph=True raises for such an optimizer."""
    ref = trajectory(kind, cdt, False, groups=groups)
    graph = trajectory(kind, cdt, True, groups=groups)
    eager = trajectory(kind, cdt, 2, groups=groups)
    assert ref["marks"] and ref["stats"] == (0, 0) and graph["stats"] == (2, 4) and eager["stats"] == (0, 0), (ref["stats"], graph["stats"])
    same_bits(graph, ref, "graph")
    same_bits(eager, ref, "prologue + eager launches")
    for run, what in ((graph, "graph"), (eager, "eager"), (ref, "unfused")):
        frozen_untouched(run, what)
    for run in (graph, eager):
        elems = int(run["mask"][: run["n"]].sum())
        assert run["frozen"] == [(elems, 2, 1)] * 4, run["frozen"]
        accounted(run)
    print("%s %s %s: %d of %d elements frozen, update %s" % (kind, cdt, groups, int(graph["mask"].sum()), graph["n"], graph["update"][-1]))


# ------------------------------------------------------------------------------------------------------ 3: the middle layer, riders
def test_frozen_middle_layer_under_riders():
    """layer 1 of 3 frozen at T = 1200, where every rider host carries: the rider cursor hops over the frozen layer.  Riders on, riders
    off and the unfused path: the same bits; ridden > 0; ridden + swept + frozen = the update range."""
    fz = (False, (1,))
    ride = trajectory("bert", torch.bfloat16, True, freeze=fz, shapes=BIG, envs=(("MB_ADAMW_RIDE", "1"), ("MB_GROUP_WGRAD", "256")))
    plain = trajectory("bert", torch.bfloat16, True, freeze=fz, shapes=BIG, envs=(("MB_ADAMW_RIDE", "0"), ("MB_GROUP_WGRAD", "256")))
    ref = trajectory("bert", torch.bfloat16, False, freeze=fz, shapes=BIG, envs=(("MB_GROUP_WGRAD", "256"),))
    same_bits(ride, ref, "riders on")
    same_bits(plain, ref, "riders off")
    for run in (ride, plain):
        frozen_untouched(run, "middle layer")
        accounted(run)
        assert all(f[1:] == (1, 0) for f in run["frozen"]), run["frozen"]
    print("middle layer frozen at T = 1200: update %s frozen %s" % (ride["update"][0], ride["frozen"][0]))
    assert ride["update"][0][0] > 0 and plain["update"][0][0] == 0


def test_frozen_layers_without_the_grouped_launch():
    """MB_GROUP_WGRAD=0, the four-launch form: the same bits, the frozen layers' launches are left out too"""
    ref = trajectory("bert", torch.bfloat16, False, envs=(("MB_GROUP_WGRAD", "0"),))
    run = trajectory("bert", torch.bfloat16, True, envs=(("MB_GROUP_WGRAD", "0"),))
    same_bits(run, ref, "four launches")
    frozen_untouched(run, "four launches")
    assert all(f[1:] == (2, 1) for f in run["frozen"]), run["frozen"]


# ------------------------------------------------------------------------------------------------------------- 4: a partial layer
def test_one_frozen_weight_of_a_layer_skips_nothing():
    """only layer 1's intermediate.dense.weight is frozen: the layer's grouped launch still runs (it produces three trainable tensors),
    the frozen tensor is left out of the update and its gradient range reads zero after every step"""
    fz = ("encoder.layer.1.intermediate.dense.weight",)
    ref = trajectory("bert", torch.bfloat16, False, freeze=fz)
    graph = trajectory("bert", torch.bfloat16, True, freeze=fz)
    eager = trajectory("bert", torch.bfloat16, 2, freeze=fz)
    same_bits(graph, ref, "graph")
    same_bits(eager, ref, "eager")
    for run in (graph, eager):
        frozen_untouched(run, "partial layer")
        accounted(run)
        assert all(f[1:] == (0, 0) and f[0] == 3072 * 768 for f in run["frozen"]), run["frozen"]


# ----------------------------------------------------------------------------------------------------- 5: embeddings, then unfreeze
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_unfreeze_mid_run(kind):
    """embeddings frozen for two updates, then model.unfreeze() and a new optimizer over everything for two more: the continuation
    equals the unfused path doing the same -- the word-row stamps start distrusted, a table that was never swept is trained again"""
    fz = (True, ())
    ref = trajectory(kind, torch.bfloat16, False, freeze=fz, thaw_at=2)
    run = trajectory(kind, torch.bfloat16, True, freeze=fz, thaw_at=2)
    same_bits(run, ref, "unfreeze")
    assert run["frozen"][:2] == [(int(run["mask"][: run["n"]].sum()), 0, 1)] * 2 and run["frozen"][2:] == [(0, 0, 0)] * 2, run["frozen"]
    assert max(run["gmax"]) == 0.0
    mask = run["mask"]
    assert not torch.equal(run["p"][mask], run["start"][mask]) and float(run["m"][mask].abs().max()) > 0.0
    only = trajectory(kind, torch.bfloat16, True, freeze=fz, nsteps=2)
    frozen_untouched(only, "embeddings only")


# ---------------------------------------------------------------------------------------------------------------- 6: accumulation
def test_accumulation_from_a_cold_start():
    """gradient accumulation of 2: the first micro-step runs before any map exists and fills the frozen ranges of the gradient buffer;
    the marks' installation clears them, and later micro-steps leave the frozen launches out"""
    ref = trajectory("bert", torch.bfloat16, False, shapes=((5, 40),), accum=2)
    run = trajectory("bert", torch.bfloat16, True, shapes=((5, 40),), accum=2)
    same_bits(run, ref, "accumulation")
    frozen_untouched(run, "accumulation")
    accounted(run)
    assert run["stats"][1] == 8 and all(f[1:] == (2, 1) for f in run["frozen"]), (run["stats"], run["frozen"])


# ------------------------------------------------------------------------------------------------------------------- 7: clipping
def f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_clipping_takes_the_norm_of_the_trainable_tensors(kind):
    """grad_clip_stats()[0] is within 1e-6 relative of the fp64 norm over the trainable tensors' gradients of a graph=False twin, read
    before its optimizer.step() (the bound and method of test_grad_clip_gpu.py); with max_grad_norm at least twice every norm the run
    equals the unclipped frozen run bit for bit"""
    cdt = torch.bfloat16
    twin = trajectory(kind, cdt, False, by_hand=True)
    hi = max(twin["norm64"])
    loose = trajectory(kind, cdt, True, max_norm=f32(2.5 * hi))
    same_bits(loose, twin, "max_grad_norm above every norm")
    frozen_untouched(loose, "clipped")
    assert len(loose["clip"]) == 4
    for (norm, coef), n64 in zip(loose["clip"], twin["norm64"]):
        print("%s update: engine norm %.9g, fp64 over the trainable .grad tensors %.9g, coef %.9g" % (kind, norm, n64, coef))
        assert abs(norm - n64) <= 1e-6 * n64 and coef == 1.0, (norm, n64, coef)
    assert all(u[0] == 0 for u in loose["update"])          # no riders under clipping
    accounted(loose)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_frozen_moments_scale_with_the_coefficient(kind):
    """one update from zero moments: clipping off, and max_norm = norm / 4.  m_clip = coef * m_off and v_clip = coef^2 * v_off to 1e-6
    on the trainable elements with |m_off| > 1e-20, as test_moments_scale_with_the_coefficient checks; frozen moments stay zero"""
    cdt = torch.bfloat16
    norm = trajectory(kind, cdt, False, by_hand=True, nsteps=1)["norm64"][0]
    off = trajectory(kind, cdt, True, nsteps=1)
    on = trajectory(kind, cdt, True, nsteps=1, max_norm=f32(norm / 4))
    (got_norm, coef), = on["clip"]
    assert abs(got_norm - norm) <= 1e-6 * norm and 0.2 < coef < 0.3, (got_norm, norm, coef)
    n, mask = on["n"], on["mask"][: on["n"]]
    m_off, v_off = off["m"][:n].double(), off["v"][:n].double()
    m_on, v_on = on["m"][:n].double(), on["v"][:n].double()
    assert float(m_on[mask].abs().max()) == 0.0 and float(v_on[mask].abs().max()) == 0.0
    keep = (m_off.abs() > 1e-20) & ~mask
    assert int(keep.sum()) > int((~mask).sum()) // 4
    c = float(np.float32(coef))
    em = ((m_on - c * m_off).abs() / m_off.abs())[keep]
    ev = ((v_on - c * c * v_off).abs() / v_off)[keep]
    print("%s: coef %.9g, %d elements, worst relative error m %.3e v %.3e" % (kind, coef, int(keep.sum()), float(em.max()), float(ev.max())))
    assert float(em.max()) <= 1e-6 and float(ev.max()) <= 1e-6


# --------------------------------------------------------------------------------------------------------------------- 8: oracle
# per-tensor bound = RATIO * the tensor's own peak group lr, logits within 5e-3: the project's bounds (test_param_groups_gpu.py)
RATIO = 2e-4 / 1e-3


def _oracle_run(kind, mode):
    layers = 2
    m = build(kind, layers, torch.float32, dropout=False).train()
    if kind == "bert":
        o = R.MAG_BertForSequenceClassification(R.BertConfigLite(num_hidden_layers=layers), R.MultimodalConfig(1.0, 0.0), 47, 74)
        o = R.set_dropout(R.load_deterministic(o, "test"), 0.0, 0.0, 0.0).train()
    else:
        o = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(n_layer=layers), X.MultimodalConfig(1.0, 0.0), 47, 74)
        o = X.set_dropout(X.load_deterministic(o, "test"), 0.0, 0.0).train()
    frozen = set(m.freeze(embeddings=True, layers=1))
    opt = AdamW(layerwise_lr_groups(m.named_parameters(), layers, LR, layer_decay=DECAY, head_lr=HEAD), lr=LR)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    # the oracle model has the same tensors left out of its optimizer
    ogroups = layerwise_lr_groups([(n, p) for n, p in o.named_parameters() if n not in frozen], layers, LR, layer_decay=DECAY, head_lr=HEAD)
    peak = {id(p): g["lr"] for g in ogroups for p in g["params"]}
    oo = O.AdamW(ogroups, lr=LR)
    so = O.get_linear_schedule_with_warmup(oo, num_warmup_steps=1.0, num_training_steps=10)
    start = {n: p.detach().clone() for n, p in o.named_parameters()}
    for s in range(3):
        m.train_step(*batch(kind, 4, 50, 50 + s), optimizer=opt, graph=mode)
        sch.step()
        i2, v2, a2, m2, s2, l2 = batch(kind, 4, 50, 50 + s, "cpu")
        o.zero_grad()
        torch.nn.functional.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1)).backward()
        oo.step(); so.step()
    torch.cuda.synchronize()
    om = dict(o.named_parameters())
    rows = []
    for n, p in m.named_parameters():
        if n in frozen or id(om[n]) not in peak:
            assert torch.equal(p.detach().cpu(), start[n]) and torch.equal(om[n].detach(), start[n]), n          # frozen: exactly equal
            continue
        rows.append((float((p.detach().cpu() - om[n].detach()).abs().max()) / (RATIO * peak[id(om[n])]), n))
    m.eval(); o.eval()
    data = batch(kind, 4, 50, 60)
    with torch.no_grad():
        l1 = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].cpu()
        i2, v2, a2, m2, s2, _ = batch(kind, 4, 50, 60, "cpu")
        l0 = o(i2, v2, a2, m2, s2)[0]
    return rows, float((l1 - l0).abs().max()), m, len(frozen)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_three_frozen_updates_track_the_oracle_fp32(kind):
    """fp32, dropout off, two layers, embeddings + layer 0 frozen, three updates through the replayed graph against
    oracle.optim_ref.AdamW over the oracle model with the same tensors left out: every trainable tensor within RATIO * its own peak
    group lr, eval logits within 5e-3, frozen tensors exactly equal.  The same comparison through graph=False runs first and is
    printed next to it: the bound is the project's existing one, never one taken from the fused run."""
    rows_u, logit_u, _, _ = _oracle_run(kind, False)
    rows_f, logit_f, m, nfrozen = _oracle_run(kind, True)
    wu, wf = max(rows_u), max(rows_f)
    print("%s frozen oracle case (%d tensors frozen): worst err / bound unfused %.3f (%s), fused %.3f (%s); logits %.2e / %.2e"
          % (kind, nfrozen, wu[0], wu[1], wf[0], wf[1], logit_u, logit_f))
    assert m._core.freeze_stats()[1:] == (1, 1) and m._core.graph_stats() == (1, 3)
    assert wu[0] <= 1.0 and logit_u <= 5e-3, (wu, logit_u)
    bad = [(r, n) for r, n in rows_f if r > 1.0]
    assert not bad and logit_f <= 5e-3, (bad, logit_f)


# ------------------------------------------------------------------------------------------------------------- 9: nothing frozen
@pytest.mark.parametrize("groups", ["driver", "classed"])
def test_nothing_frozen_installs_no_marks(groups):
    run = trajectory("bert", torch.bfloat16, True, freeze=None, groups=groups, nsteps=2)
    assert not run["marks"] and run["frozen"] == [(0, 0, 0)] * 2 and all(u[0] + u[1] == run["n"] for u in run["update"])


# ------------------------------------------------------------------------------------------------------------------ 10: the driver
@pytest.mark.parametrize("model", ["bert-base-uncased", "xlnet-base-cased"])
def test_driver_epoch_with_frozen_layers(model, monkeypatch, capsys):
    """--synthetic 96 --n_epochs 1 --freeze_layers 2 --freeze_embeddings with the model's configuration cut to 3 layers: the epoch
    finishes with a finite loss, every update went through the single call, and the run reports what it left out"""
    import json
    from bert_multimodal_transformer_amd import multimodal_driver as D
    monkeypatch.setattr(D, "bert_config", lambda model, num_labels=1: BertConfig(num_hidden_layers=3, num_labels=num_labels))
    monkeypatch.setattr(D, "xlnet_config", lambda model, num_labels=1: XLNetConfig(n_layer=3, num_labels=num_labels))
    old = getattr(D, "args", None)
    try:
        D.main(["--model", model, "--synthetic", "96", "--n_epochs", "1", "--freeze_layers", "2", "--freeze_embeddings", "--seed", "5"])
    finally:
        D.args = old
    recs = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    left_out = [r for r in recs if "wgrad_launches_skipped" in r]
    assert len(left_out) == 1 and left_out[0]["wgrad_launches_skipped"] == 2 and left_out[0]["embed_backward_skipped"] == 1
    assert left_out[0]["frozen_params"] > 20e6
    final = [r for r in recs if "train_loss" in r]
    assert len(final) == 1 and math.isfinite(final[0]["train_loss"]) and final[0]["train_samples_per_sec"] > 0
