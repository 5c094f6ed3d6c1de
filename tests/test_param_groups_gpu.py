"""GPU: per-group AdamW hyper-parameters (update classes) in the single-call training step.

The groups under test come from optimization.layerwise_lr_groups with layer_decay = 0.5 and head_lr = 5 * lr: neighbouring classes
differ by a factor of two, the head by forty against the embeddings -- a tensor updated with a neighbour's class cannot hide.  The
yardstick is the path that handled any groups before: train_step(..., graph=False) = training_step + optimizer.step(); in
deterministic mode the fused step equals it bit for bit, as the two-group step does (test_model_gpu.py).  One case compares with the
CPU oracle's optimizer over the oracle model, which shares no line with the code under test."""
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


def batch(kind, B, L, seed, dev=DEV):
    b = (weights.synthetic_bert_batch if kind == "bert" else weights.synthetic_xlnet_batch)(B, L, 47, 74, seed=seed)
    t = lambda k: torch.from_numpy(b[k]).to(dev)
    return t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"), t("label_ids")


def classed_groups(named, layers):
    return layerwise_lr_groups(named, layers, LR, layer_decay=DECAY, head_lr=HEAD)


def trajectory(kind, cdt, mode, shapes=SMALL, nsteps=4, accum=1, layers=3, groups="classed", halve=None, zero_group=None):
    """nsteps optimizer updates (dropout on, schedule moving) through model.train_step.  mode: False = training_step + optimizer.step(),
    True = step prologue + replayed graph, 2 = prologue + the same kernels launched one by one.  halve = (update, group): that group's lr
    is halved by hand before that update; zero_group: that group starts -- and so stays -- at lr 0."""
    torch.manual_seed(77)
    m = build(kind, layers, cdt).train()
    gs = classed_groups(m.named_parameters(), layers) if groups == "classed" else optimizer_grouped_parameters(m)
    if zero_group is not None:
        gs[zero_group]["lr"] = 0.0
    opt = AdamW(gs, lr=LR)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    start = m.flat_params.clone()
    stats_after = {}
    with m.stream_scope():
        for s in range(nsteps * accum):
            B, L = shapes[s % len(shapes)]
            data = batch(kind, B, L, 90 + s)
            update = (s + 1) % accum == 0
            if halve is not None and update and (s + 1) // accum - 1 == halve[0]:
                opt.param_groups[halve[1]]["lr"] *= 0.5
            if mode == 2:
                core = m._core
                o = opt.flat_step_args(core) if update else None
                if update:
                    opt._t += 1
                    o["t"] = opt._t
                core.train_step(*data, o, loss_scale=1.0 / accum, mode=2)
            else:
                m.train_step(*data, optimizer=opt if update else None, loss_scale=1.0 / accum, graph=mode)
            if update:
                sch.step()
                if mode is not False:
                    stats_after[(B, L)] = m._core.update_stats()
    stats = m._core.graph_stats()
    m.eval()
    data = batch(kind, 4, 40, 99)
    with torch.no_grad():
        logits = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].clone()
    torch.cuda.synchronize()
    out = dict(p=m.flat_params.clone(), m=m._core._adam_m.clone(), v=m._core._adam_v.clone(), g=m.flat_grads.clone(), logits=logits,
               shadow=m._core.shadow.clone(), stats=stats, update=stats_after, start=start, model=m, opt=opt)
    if kind == "xlnet":
        out["frozen"] = m.transformer.mask_emb.detach().clone()
    return out


def same_bits(run, ref, what):
    for k in ("p", "m", "v", "shadow", "logits"):
        assert torch.equal(run[k], ref[k]), "%s: %s differs, max %.3e" % (what, k, float((run[k].float() - ref[k].float()).abs().max()))
    assert float(run["g"].abs().max()) == 0.0, what


@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float32])
def test_classed_fused_step_equals_the_unfused_path_bit_for_bit(cdt, monkeypatch):
    """MAG-BERT, layer-wise groups, four updates over two shapes: the replayed graph and the prologue + eager launches end every tensor
    -- parameters, both moments, the bf16 shadow, the eval logits of a fifth batch -- on the bits of training_step + optimizer.step().
    One group's lr is halved by hand before the third update: values travel with the step prologue, so still two captures."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    halve = (2, 5)
    ref = trajectory("bert", cdt, False, halve=halve)
    graph = trajectory("bert", cdt, True, halve=halve)
    eager = trajectory("bert", cdt, 2, halve=halve)
    assert ref["stats"] == (0, 0) and graph["stats"] == (2, 4) and eager["stats"] == (0, 0), (ref["stats"], graph["stats"], eager["stats"])
    same_bits(graph, ref, "graph")
    same_bits(eager, ref, "prologue + eager launches")
    segs = graph["update"][(5, 40)][2]
    assert segs == len(graph["opt"]._class_map(graph["model"]._core)[1]) > 2


def test_classed_riders_in_every_host(monkeypatch):
    """T = 1,200 (B = 24, L = 50), where every host carries riders: with a map their slices are clamped to the segment of their top
    element and read that class's slot.  Riders on, riders off and the unfused path: the same bits; the getter splits the update."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    monkeypatch.setenv("MB_GROUP_WGRAD", "256")
    shapes = ((24, 50), (24, 50), (5, 40), (24, 50))
    monkeypatch.setenv("MB_ADAMW_RIDE", "1")
    ride = trajectory("bert", torch.bfloat16, True, shapes=shapes)
    monkeypatch.setenv("MB_ADAMW_RIDE", "0")
    plain = trajectory("bert", torch.bfloat16, True, shapes=shapes)
    ref = trajectory("bert", torch.bfloat16, False, shapes=shapes)
    same_bits(ride, ref, "classed, riders on")
    same_bits(plain, ref, "classed, riders off")
    n = ride["model"]._core.n_update_end
    ridden, swept, segs = ride["update"][(24, 50)]
    print("classed step at T = 1200: ridden %d swept %d of %d, %d segments" % (ridden, swept, n, segs))
    assert ridden > 0 and ridden + swept == n and segs > 2
    assert plain["update"][(24, 50)][:2] == (0, n)


def test_classed_gradient_accumulation(monkeypatch):
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ref = trajectory("bert", torch.bfloat16, False, shapes=((5, 40),), accum=2)
    run = trajectory("bert", torch.bfloat16, True, shapes=((5, 40),), accum=2)
    same_bits(run, ref, "accumulation")
    assert run["stats"] == (2, 8)                                                  # one graph with the update, one without


def test_a_group_at_lr_zero_keeps_its_bits(monkeypatch):
    """lr = 0 is the supported way to freeze a group: full compute, the moments move, the parameters keep their exact bits."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    k = 4                                                                          # layer 1's decayed tensors (GEMM weights)
    ref = trajectory("bert", torch.bfloat16, False, zero_group=k)
    run = trajectory("bert", torch.bfloat16, True, zero_group=k)
    same_bits(run, ref, "lr = 0 group")
    frozen = [p for p in run["opt"].param_groups[k]["params"]]
    assert frozen and run["opt"].param_groups[k]["lr"] == 0.0
    touched = torch.zeros_like(run["p"], dtype=torch.bool)
    for p in frozen:
        _, off, numel, _ = p._mb_flat
        touched[off: off + numel] = True
        assert torch.equal(run["p"][off: off + numel], run["start"][off: off + numel])
        assert float(run["m"][off: off + numel].abs().max()) > 0.0 and float(run["v"][off: off + numel].abs().max()) > 0.0
    assert not torch.equal(run["p"][~touched], run["start"][~touched])


def test_classed_xlnet_step(monkeypatch):
    """MAG-XLNet at the shapes of test_xlnet_adamw_riders_change_nothing: riders on, riders off (one table-driven sweep launch either
    way) and the unfused path end on the same bits; the frozen mask_emb slot is untouched."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    shapes = ((24, 50), (24, 50), (5, 40), (24, 50))
    monkeypatch.setenv("MB_ADAMW_RIDE", "1")
    ride = trajectory("xlnet", torch.bfloat16, True, shapes=shapes)
    monkeypatch.setenv("MB_ADAMW_RIDE", "0")
    plain = trajectory("xlnet", torch.bfloat16, True, shapes=shapes)
    ref = trajectory("xlnet", torch.bfloat16, False, shapes=shapes)
    same_bits(ride, ref, "xlnet classed, riders on")
    same_bits(plain, ref, "xlnet classed, riders off")
    assert ride["stats"] == plain["stats"] == (2, 4)
    core = ride["model"]._core
    mask0 = torch.from_numpy(weights.make_param("transformer.mask_emb", tuple(ride["frozen"].shape), "test")).to(DEV)
    assert torch.equal(ride["frozen"], mask0) and torch.equal(plain["frozen"], mask0) and torch.equal(ref["frozen"], mask0)
    ridden, swept, segs = ride["update"][(24, 50)]
    print("xlnet classed step at T = 1200: ridden %d swept %d of %d, %d segments" % (ridden, swept, core.n_update_end, segs))
    assert ridden + swept == core.n_update_end and segs > 2 and plain["update"][(24, 50)][:2] == (0, core.n_update_end)


# per-tensor bound of the oracle case = RATIO * the tensor's own peak group lr: the project's bound for this comparison, 2e-4 at
# lr 1e-3 (test_three_optimizer_steps_track_the_oracle_fp32: Adam's sign flips on near-zero gradients, which scale with lr)
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
    opt = AdamW(classed_groups(m.named_parameters(), layers), lr=LR)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    ogroups = classed_groups(o.named_parameters(), layers)
    peak = {}
    for g in ogroups:
        for p in g["params"]:
            peak[id(p)] = g["lr"]
    oo = O.AdamW(ogroups, lr=LR)
    so = O.get_linear_schedule_with_warmup(oo, num_warmup_steps=1.0, num_training_steps=10)
    for s in range(3):
        m.train_step(*batch(kind, 4, 50, 50 + s), optimizer=opt, graph=mode)
        sch.step()
        i2, v2, a2, m2, s2, l2 = batch(kind, 4, 50, 50 + s, "cpu")
        oo.zero_grad()
        torch.nn.functional.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1)).backward()
        oo.step(); so.step()
    torch.cuda.synchronize()
    om = dict(o.named_parameters())
    rows = []
    for n, p in m.named_parameters():
        if om[n].grad is None:
            assert torch.equal(p.detach().cpu(), om[n].detach()), n
            continue
        rows.append((float((p.detach().cpu() - om[n].detach()).abs().max()) / (RATIO * peak[id(om[n])]), n))
    m.eval(); o.eval()
    data = batch(kind, 4, 50, 60)
    with torch.no_grad():
        l1 = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].cpu()
        i2, v2, a2, m2, s2, _ = batch(kind, 4, 50, 60, "cpu")
        l0 = o(i2, v2, a2, m2, s2)[0]
    return rows, float((l1 - l0).abs().max()), m


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_three_classed_updates_track_the_oracle_fp32(kind):
    """fp32, dropout off, two layers, three classed updates through the replayed graph against oracle.optim_ref.AdamW over the oracle
    model with the same groups (layerwise_lr_groups fed the oracle's own named_parameters): every tensor within RATIO * its own peak
    group lr, eval logits within 5e-3.  The same comparison through graph=False -- code this feature does not touch -- runs first and
    is printed next to it: the bound is the project's existing one, never one taken from the fused run.  Measured, worst tensor as a
    fraction of its bound (the word-embedding table both times): MAG-BERT unfused 0.032, fused 0.040; MAG-XLNet unfused 0.012, fused
    0.011 -- the unfused path stays inside the existing ratio at every class's lr, so no tensor needed a bound of its own."""
    rows_u, logit_u, _ = _oracle_run(kind, False)
    rows_f, logit_f, m = _oracle_run(kind, True)
    wu, wf = max(rows_u), max(rows_f)
    print("%s oracle case: worst err / bound unfused %.3f (%s), fused %.3f (%s); logits %.2e / %.2e" % (kind, wu[0], wu[1], wf[0], wf[1], logit_u, logit_f))
    assert m._core.update_stats()[2] > 2 and m._core.graph_stats() == (1, 3)
    assert wu[0] <= 1.0 and logit_u <= 5e-3, (wu, logit_u)
    bad = [(r, n) for r, n in rows_f if r > 1.0]
    assert not bad and logit_f <= 5e-3, (bad, logit_f)


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_the_two_group_optimizer_installs_no_map(kind, monkeypatch):
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ref = trajectory(kind, torch.bfloat16, False, groups="driver")
    run = trajectory(kind, torch.bfloat16, True, groups="driver")
    same_bits(run, ref, "two groups")
    args = run["opt"].flat_step_args(run["model"]._core)
    assert args is not None and "map" not in args and "classes" not in args and run["stats"] == (2, 4)
    assert all(u[2] == 0 for u in run["update"].values()) and run["model"]._core.update_stats()[2] == 0


def test_a_refused_map_leaves_the_previous_one_in_force(monkeypatch):
    """an unsorted boundary and a boundary that is no tensor offset are refused with the error code; the step that follows still runs
    under the map installed before, and ends where the unfused path ends.  The data-parallel forms decline a classed optimizer."""
    import ctypes as C
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ref = trajectory("bert", torch.bfloat16, False, nsteps=2)
    torch.manual_seed(77)
    m = build("bert", 3, torch.bfloat16).train()
    opt = AdamW(classed_groups(m.named_parameters(), 3), lr=LR)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    core = m._core
    assert opt.flat_step_args(core, allow_dp=True) is not None          # (no data parallel here: allow_dp changes nothing)
    opt._dp = object()
    assert opt.flat_step_args(core, allow_dp=True) is None and opt.flat_step_args(core) is None
    opt._dp = None
    with m.stream_scope():
        m.train_step(*batch("bert", 5, 40, 90), optimizer=opt, graph=True)
        sch.step()
        bounds, classes = opt.flat_step_args(core)["map"]
        nseg = core.update_stats()[2]
        assert nseg == len(classes)
        L = _lib.lib()
        bad = list(bounds)
        bad[1], bad[2] = bad[2], bad[1]
        for wrong in (bad, [bounds[0], bounds[1] + 4] + list(bounds[2:])):
            code = L.mb_bert_set_update_map(core.handle, max(classes) + 1, len(classes), (C.c_size_t * len(wrong))(*wrong),
                                            (C.c_int * len(classes))(*classes))
            assert code == 1001, code
        assert L.mb_bert_train_step_dp(core.handle, None, None, None, None, None, None, 5, 40, 0, 1, None, None, None, None, None, 1e-3, 0.9,
                                       0.999, 1e-6, 0.01, 1, 1, 1.0, 1.0, 1, None, None) == 1002
        m.train_step(*batch("bert", 5, 40, 91), optimizer=opt, graph=True)
        sch.step()
    torch.cuda.synchronize()
    assert core.update_stats()[2] == nseg and core.graph_stats() == (1, 2)
    assert torch.equal(m.flat_params, ref["p"]) and torch.equal(core._adam_m, ref["m"]) and torch.equal(core._adam_v, ref["v"])
