"""GPU: MAG-BERT with the Multimodal Adaptation Gate in front of encoder layer j (injection_index) on every path the model has.

References: tests/golden/g14_bert_injection.npz (the reference's own modules composed in the moved order: scripts/make_golden_injection.py)
and the CPU oracle with patch_oracle(o, j) run live on the same inputs.  Bounds are the project's existing ones (test_model_gpu,
test_bert_sizes_gpu, test_freeze_gpu, test_dp_gpu): fp32 logits 1e-3 and gradients 5e-3 of the tensor's max, bf16 logits 1e-2 and
gradients 3e-2 relative Frobenius (MAG's gated tensors 1e-1), bit-identical trajectories across the step paths in deterministic mode."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, BertConfig, MAG_BertForSequenceClassification, MAG_BertModel, MultimodalConfig,
                                             XLNetConfig, get_linear_schedule_with_warmup, rng)
from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
from conftest import free_port
from oracle import mag_bert_ref as R, optim_ref as O, weights
from test_dp_gpu import _ENGINE_WORKER
from test_freeze_gpu import BIG, LR, SMALL, accounted, apply_freeze, batch, env, frozen_mask, frozen_untouched, make_groups, same_bits
from test_model_gpu import DEV, LOOSE_BF16, _Replay, _grad_report, tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_injection import A_DIM, CASES, INDICES, SAMPLE, SEED, key, patch_oracle, size_kw      # noqa: E402

SMALL_KW = size_kw()                                     # 3 layers x 256 wide, 4 heads, inner 1024: the fixture's model
del SMALL_KW["num_labels"]


def make(j, cdt=torch.float32, V=47, kw=None, layers=3, p=0.0, p_mag=0.0, max_seq_length=None, cls=MAG_BertForSequenceClassification):
    """kw = None: default BertConfig (768 wide) with `layers` layers; SMALL_KW: the fixture's model.  j = None: built without the argument"""
    cfg = BertConfig(num_labels=1, hidden_dropout_prob=p, attention_probs_dropout_prob=p, **(dict(num_hidden_layers=layers) if kw is None else kw))
    extra = {} if j is None else {"injection_index": j}
    m = cls(cfg, MultimodalConfig(1.0, p_mag), visual_dim=V, acoustic_dim=A_DIM, compute_dtype=cdt, max_seq_length=max_seq_length, **extra)
    pre = "" if cls is MAG_BertForSequenceClassification else "bert."
    m.load_state_dict({n: torch.from_numpy(weights.make_param(pre + n, tuple(q.shape), "test")) for n, q in m.named_parameters()})
    return m


def oracle(j, V=47, kw=None, layers=3, p=0.0, p_mag=0.0):
    o = R.MAG_BertForSequenceClassification(R.BertConfigLite(**(dict(num_hidden_layers=layers) if kw is None else kw)),
                                            R.MultimodalConfig(1.0, p_mag), V, A_DIM)
    o = R.set_dropout(R.load_deterministic(o, "test"), p, p, p_mag)
    return o if j is None else patch_oracle(o, j)


def mse_backward(model, data, **kw):
    ids, vis, aco, mask, seg, lab = data
    logits = model(ids, vis, aco, attention_mask=mask, token_type_ids=seg, **kw)[0]
    loss = torch.nn.functional.mse_loss(logits.view(-1), lab.view(-1))
    loss.backward()
    return logits.detach(), float(loss)


def bf16_loss_bound(ref_logits, labels, eps=1e-2):
    """what the project's bf16 logit bound (1e-2) allows the MSE loss to move: with residuals r_i = logit_i - label_i of the reference
    and every logit off by at most eps, |mean((r_i + d_i)^2) - mean(r_i^2)| <= mean(2 |r_i| eps + eps^2)"""
    r = (ref_logits.view(-1) - labels.view(-1)).abs()
    return float((2.0 * r * eps + eps * eps).mean())


# ------------------------------------------------------------------------------------------------------------- 1: eval parity
@pytest.mark.parametrize("j", INDICES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_L%d_V%d" % c)
def test_eval_logits_and_sequence_output(golden, j, case):
    g = golden["g14_bert_injection"]
    B, L, V = case
    b = weights.synthetic_bert_batch(B, L, V, A_DIM, seed=SEED)
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    o = oracle(j, V, SMALL_KW, p_mag=0.5).eval()
    i2, v2, a2, m2, s2, _ = tb(b)
    with torch.no_grad():
        live = o(i2, v2, a2, m2, s2)[0]
        live_seq = o.bert(i2, v2, a2, m2, s2)[0]
    m = make(j, torch.float32, V, SMALL_KW, p=0.1, p_mag=0.5).eval()
    with torch.no_grad():
        got = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].cpu()
    seq = m._core.sequence_output(B, L).float().cpu()
    err = float(np.abs(got.numpy() - g[key("logits", j, case)]).max())
    err_seq = float(np.abs(weights.strided_sample(seq.numpy(), SAMPLE) - g[key("seq", j, case)]).max())
    err_live, err_live_seq = float((got - live).abs().max()), float((seq - live_seq).abs().max())
    mb = make(j, torch.bfloat16, V, SMALL_KW, p=0.1, p_mag=0.5).eval()
    with torch.no_grad():
        got16 = mb(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].float().cpu()
    err16 = max(float(np.abs(got16.numpy() - g[key("logits", j, case)]).max()), float((got16 - live).abs().max()))
    print("j=%d %s fp32: logits vs fixture %.3e, vs live oracle %.3e; sequence output sample %.3e, whole vs live %.3e; bf16 logits %.3e"
          % (j, case, err, err_live, err_seq, err_live_seq, err16))
    assert err <= 1e-3 and err_live <= 1e-3 and err_seq <= 1e-3 and err_live_seq <= 1e-3
    assert err16 <= 1e-2


# ---------------------------------------------------------------------------------------------------------- 2: fp32 gradients
@pytest.mark.parametrize("j", INDICES)
def test_gradients_fp32(j):
    """train mode, every dropout p = 0, B = 4, L = 50: loss and all gradients against the patched oracle; the fused training_step and
    train_step(optimizer=None) give the autograd path's gradients"""
    m = make(j, kw=SMALL_KW).train()
    o = oracle(j, kw=SMALL_KW).train()
    b = weights.synthetic_bert_batch(4, 50, 47, A_DIM, seed=21)
    _, loss = mse_backward(m, tb(b, DEV))
    _, lo = mse_backward(o, tb(b))
    torch.cuda.synchronize()
    print("j=%d fp32 loss %.6f vs oracle %.6f" % (j, loss, lo))
    assert abs(loss - lo) < 1e-4
    _grad_report(m, o, 5e-3, show=3)
    g_ref = m.flat_grads.clone()
    for step in (lambda: m.training_step(*tb(b, DEV)), lambda: m.train_step(*tb(b, DEV), optimizer=None)):
        m.zero_grad()
        l2 = step()
        torch.cuda.synchronize()
        assert abs(float(l2) - loss) < 1e-5
        assert float((m.flat_grads - g_ref).abs().max()) <= 1e-5 * float(g_ref.abs().max()) + 1e-9


# ---------------------------------------------------------------------------------------------------------- 3: bf16 gradients
@pytest.mark.parametrize("j", INDICES)
def test_gradients_bf16(j):
    """3 x 768, B = 4, L = 50, dropout off: 3e-2 relative Frobenius for every tensor, MAG's four gated weights 1e-1.  The tensors below
    the gate receive their gradient through the gate's relu here.  Measured values: profiles/injection_errors.txt"""
    m = make(j, torch.bfloat16).train()
    o = oracle(j).train()
    b = weights.synthetic_bert_batch(4, 50, 47, A_DIM, seed=21)
    loss = m.training_step(*tb(b, DEV))
    ref_logits, lo = mse_backward(o, tb(b))
    torch.cuda.synchronize()
    bound = bf16_loss_bound(ref_logits, tb(b)[5])
    print("j=%d bf16 loss %.5f vs oracle %.5f (bound %.2e)" % (j, float(loss), lo, bound))
    assert abs(float(loss) - lo) <= bound
    _grad_report(m, o, 3e-2, frobenius=True, loose=LOOSE_BF16, tol_loose=1e-1, show=8)


# ------------------------------------------------------------------------------------------------------ 4: dropout mask replay
@pytest.mark.parametrize("cdt,tol_logit,tol_grad", [(torch.float32, 1e-3, 5e-3), (torch.bfloat16, 1e-2, 3e-2)])
def test_train_mode_dropout_mask_replay(cdt, tol_logit, tol_grad):
    """2 x 768, B = 3, L = 24, j = 1, dropout 0.1 / 0.1 / MAG 0.5: the device masks regenerated on the host and replayed inside the
    patched oracle.  MAG's mask multiplies the output of layer 0 now; its site key is SITE_MAG as before."""
    j, layers, B, L, V, nh, H = 1, 2, 3, 24, 47, 12, 768
    torch.manual_seed(99)
    m = make(j, cdt, layers=layers, p=0.1, p_mag=0.5).train()
    o = oracle(j, layers=layers, p=0.1, p_mag=0.5).train()
    core = m._core
    b = weights.synthetic_bert_batch(B, L, V, A_DIM, seed=41)
    logits, _ = mse_backward(m, tb(b, DEV))
    seed, step = core.seed, core.step
    mult = lambda site, p, n: torch.from_numpy(rng.keep_mult(n, rng.make_key(seed, step, site, p)))
    T = B * L
    o.bert.embeddings.dropout = _Replay(mult(rng.SITE_EMB, 0.1, T * H))
    o.bert.MAG.dropout = _Replay(mult(rng.SITE_MAG, 0.5, T * H))
    o.dropout = _Replay(mult(rng.SITE_HEAD, 0.1, B * H))
    for l, lyr in enumerate(o.bert.encoder.layer):
        lyr.attention.self.dropout = _Replay(mult(rng.SITE_LAYER0 + 4 * l + 0, 0.1, B * nh * L * L))
        lyr.attention.output.dropout = _Replay(mult(rng.SITE_LAYER0 + 4 * l + 1, 0.1, T * H))
        lyr.output.dropout = _Replay(mult(rng.SITE_LAYER0 + 4 * l + 2, 0.1, T * H))
    lo, _ = mse_backward(o, tb(b))
    torch.cuda.synchronize()
    err = float((logits.cpu() - lo).abs().max())
    print("j=1 train-mode logits max|err| (%s): %.3e" % (cdt, err))
    assert err <= tol_logit
    _grad_report(m, o, tol_grad, frobenius=(cdt == torch.bfloat16), loose=LOOSE_BF16 + ("classifier.bias",), tol_loose=1e-1, show=4)


# ------------------------------------------------------------------------------------------------------- 5: optional surfaces
def test_optional_surfaces_fp32():
    """j = 1, fp32, the fixture's model: hidden_states (entry i = the tensor layer i reads, so entry 1 is the gate's output), the
    differentiable base model with a gradient handed in, inputs_embeds with its gradient, a 2-D head_mask, and one tiled-attention case"""
    j, layers, B, L, V, nh, H = 1, 3, 4, 24, 47, 4, 256
    base = make(j, kw=SMALL_KW, cls=MAG_BertModel).train()
    o = oracle(j, kw=SMALL_KW).train()
    b = weights.synthetic_bert_batch(B, L, V, A_DIM, seed=81)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    i2, v2, a2, m2, s2, l2 = tb(b)
    seq, pooled, hs = base(ids, vis, aco, attention_mask=mask, token_type_ids=seg, output_hidden_states=True)
    assert seq.requires_grad and pooled.requires_grad and len(hs) == layers + 1
    w_seq = torch.from_numpy(weights.make_param("probe.seq", (H,), "test")).to(DEV)
    w_pool = torch.from_numpy(weights.make_param("probe.pool", (H,), "test")).to(DEV)
    ((seq * w_seq).sum(-1).mean() + 3.0 * (pooled * w_pool).sum(-1).mean()).backward()
    so, po = o.bert(i2, v2, a2, m2, s2)
    ((so * w_seq.cpu()).sum(-1).mean() + 3.0 * (po * w_pool.cpu()).sum(-1).mean()).backward()
    torch.cuda.synchronize()
    ref_h = o.bert.layer_inputs
    assert float((seq.detach().cpu() - so.detach()).abs().max()) <= 1e-4 and float((pooled.detach().cpu() - po.detach()).abs().max()) <= 1e-4
    for i, (h, r) in enumerate(zip(hs, ref_h)):
        assert float((h.cpu() - r.detach()).abs().max()) <= 1e-4, i
    # entry 1 is the gate's OUTPUT: it differs from what layer 0 wrote by the gate's shift
    assert float((ref_h[1].detach() - o.bert.encoder.layer[0](ref_h[0], (1.0 - m2[:, None, None, :].float()) * -10000.0).detach()).abs().max()) > 1e-2
    og = {n: p.grad for n, p in o.bert.named_parameters()}
    gmax = max(float(g.abs().max()) for g in og.values())
    rows = sorted(((float((p.grad.cpu() - og[n]).abs().max()) / max(float(og[n].abs().max()), 1e-3 * gmax), n) for n, p in base.named_parameters()),
                  reverse=True)
    print("j=1 base-model gradients through the autograd edge: worst", ["%.2e %s" % r for r in rows[:3]])
    assert rows[0][0] <= 2e-3

    # inputs_embeds (+ its gradient) and a 2-D head_mask through the classification model
    m = make(j, kw=SMALL_KW).train()
    o = oracle(j, kw=SMALL_KW).train()
    hm = torch.ones(layers, nh)
    hm[0, 3] = 0.0; hm[1, 1] = 0.5; hm[2, 0] = 0.0; hm[2, 2] = 2.0
    emb_cpu = (o.bert.embeddings.word_embeddings(i2).detach() + 0.05 * torch.from_numpy(weights.make_param("probe.emb", (B, L, H), "test"))).requires_grad_(True)
    emb = emb_cpu.detach().to(DEV).requires_grad_(True)
    logits, _ = mse_backward(m, (None, vis, aco, mask, seg, lab), head_mask=hm.to(DEV), inputs_embeds=emb)
    lo, _ = mse_backward(o, (None, v2, a2, m2, s2, l2), head_mask=hm, inputs_embeds=emb_cpu)
    torch.cuda.synchronize()
    gerr = float((emb.grad.cpu() - emb_cpu.grad).norm() / emb_cpu.grad.norm())
    err = float((logits.cpu() - lo).abs().max())
    print("j=1 head_mask + inputs_embeds: logits %.2e, d(inputs_embeds) rel. Frobenius %.2e" % (err, gerr))
    assert err <= 1e-3 and gerr <= 2e-3
    o.bert.embeddings.word_embeddings.weight.grad = torch.zeros_like(o.bert.embeddings.word_embeddings.weight)
    _grad_report(m, o, 5e-3, show=3)

    # L = 200: the tiled attention kernels
    V2 = 35
    ml = make(j, V=V2, kw=SMALL_KW, p=0.1, p_mag=0.5, max_seq_length=256).eval()
    ol = oracle(j, V2, SMALL_KW, p_mag=0.5).eval()
    bl = weights.synthetic_bert_batch(2, 200, V2, A_DIM, seed=13)
    ids, vis, aco, mask, seg, _ = tb(bl, DEV)
    i2, v2, a2, m2, s2, _ = tb(bl)
    with torch.no_grad():
        errl = float((ml(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].cpu() - ol(i2, v2, a2, m2, s2)[0]).abs().max())
    print("j=1 L=200 eval logits max|err| %.3e" % errl)
    assert errl <= 1e-3


# --------------------------------------------------------------------------------------------------------- 6: stale pad rows
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_pad_rows_of_the_pre_gate_tensor_are_cleared(cdt):
    """a step at (4, 50), then one at (3, 20): T = 60, so rows 60 - 63 of the pre-gate buffer -- the k-major `text` operand of MAG's
    weight gradient -- still hold tokens of the first batch unless the pass set-up clears them (MAG.W_hv / W_ha off by O(1))"""
    fp32 = cdt == torch.float32
    kw = SMALL_KW if fp32 else None
    m = make(1, cdt, kw=kw).train()
    o = oracle(1, kw=kw).train()
    m.training_step(*tb(weights.synthetic_bert_batch(4, 50, 47, A_DIM, seed=21), DEV))
    m.zero_grad()
    b = weights.synthetic_bert_batch(3, 20, 47, A_DIM, seed=22)
    loss = m.training_step(*tb(b, DEV))
    ref_logits, lo = mse_backward(o, tb(b))
    torch.cuda.synchronize()
    bound = 1e-4 if fp32 else bf16_loss_bound(ref_logits, tb(b)[5])
    print("j=1 second batch (%s) loss %.5f vs oracle %.5f (bound %.2e)" % (cdt, float(loss), lo, bound))
    assert abs(float(loss) - lo) <= bound
    if fp32:
        _grad_report(m, o, 5e-3, show=3)
    else:
        _grad_report(m, o, 3e-2, frobenius=True, loose=LOOSE_BF16, tol_loose=1e-1, show=3)


# ------------------------------------------------------------------------------------------- 7 / 8: every step path, the same bits
@functools.lru_cache(maxsize=None)
def trajectory(j, cdt, mode, shapes=SMALL, nsteps=4, accum=1, layers=3, freeze=None, groups="driver", max_norm=None, envs=()):
    """test_freeze_gpu.trajectory for a model built with injection_index = j (None: without the argument): nsteps updates, dropout on,
    schedule moving, deterministic mode.  mode: False = training_step + optimizer.step(), True = replayed graph, 2 = prologue + launches"""
    with env(MB_DETERMINISTIC=1, **dict(envs)):
        torch.manual_seed(77)
        m = make(j, cdt, layers=layers, p=0.1, p_mag=0.5).train()
        names = apply_freeze(m, freeze)
        opt = AdamW(make_groups(m, groups, layers), lr=LR, max_grad_norm=max_norm)
        sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
        core = m._core
        start = m.flat_params.clone()
        mask = frozen_mask(m, names)
        upd, frz, gmax, gfrozen, clip = [], [], [], [], []
        with m.stream_scope():
            for s in range(nsteps * accum):
                B, L = shapes[s % len(shapes)]
                data = batch("bert", B, L, 90 + s, label_mult=8.0 if max_norm is not None and (s // accum) % 2 == 1 else 1.0)
                update = (s + 1) % accum == 0
                if mode == 2:
                    a = opt.flat_step_args(core) if update else None
                    if update:
                        opt._t += 1
                        a["t"] = opt._t
                    core.train_step(*data, a, loss_scale=1.0 / accum, mode=2)
                    if update and a.get("max_grad_norm"):
                        opt._clip_last = core
                else:
                    m.train_step(*data, optimizer=opt if update else None, loss_scale=1.0 / accum, graph=mode)
                if update:
                    sch.step()
                    if opt.max_grad_norm:
                        clip.append(opt.last_grad_clip)
                    if mode is not False:
                        upd.append(core.update_stats())
                        frz.append(core.freeze_stats())
                        gmax.append(float(m.flat_grads.abs().max()))
                        gfrozen.append(float(m.flat_grads[mask].abs().max()) if bool(mask.any()) else 0.0)
        stats = core.graph_stats()
        m.eval()
        data = batch("bert", 4, 40, 99)
        with torch.no_grad():
            logits = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].clone()
        torch.cuda.synchronize()
        return dict(p=m.flat_params.clone(), m=core._adam_m.clone(), v=core._adam_v.clone(), logits=logits, shadow=core.shadow.clone(),
                    stats=stats, update=upd, frozen=frz, gmax=gmax, gfrozen=gfrozen, clip=clip, start=start, mask=mask, n=core.n_update_end,
                    sh=(core.sh_begin, core.sh_end))


@pytest.mark.parametrize("j,cdt", [(1, torch.bfloat16), (1, torch.float32), (2, torch.bfloat16)])
def test_every_step_path_ends_on_the_same_bits(j, cdt):
    ref = trajectory(j, cdt, False)
    graph = trajectory(j, cdt, True)
    eager = trajectory(j, cdt, 2)
    assert ref["stats"] == (0, 0) and graph["stats"] == (2, 4) and eager["stats"] == (0, 0), (ref["stats"], graph["stats"])
    same_bits(graph, ref, "graph")
    same_bits(eager, ref, "prologue + eager launches")
    assert not torch.equal(ref["p"], ref["start"])
    if cdt == torch.bfloat16:          # the position of the gate is part of the model: another index, another trajectory
        assert not torch.equal(ref["logits"], trajectory(3 - j, cdt, False)["logits"])


def test_riders_the_four_launch_form_and_accumulation_change_nothing():
    ride = trajectory(1, torch.bfloat16, True, shapes=BIG, envs=(("MB_ADAMW_RIDE", "1"), ("MB_GROUP_WGRAD", "256")))
    plain = trajectory(1, torch.bfloat16, True, shapes=BIG, envs=(("MB_ADAMW_RIDE", "0"), ("MB_GROUP_WGRAD", "256")))
    ref = trajectory(1, torch.bfloat16, False, shapes=BIG, envs=(("MB_GROUP_WGRAD", "256"),))
    same_bits(ride, ref, "riders on")
    same_bits(plain, ref, "riders off")
    print("j=1 at T = 1200: update %s (riders on), %s (off)" % (ride["update"][0], plain["update"][0]))
    assert ride["update"][0][0] > 0 and plain["update"][0][0] == 0
    for run in (ride, plain):
        assert all(u[0] + u[1] == run["n"] for u in run["update"])
    four = trajectory(1, torch.bfloat16, True, envs=(("MB_GROUP_WGRAD", "0"),))
    same_bits(four, trajectory(1, torch.bfloat16, False, envs=(("MB_GROUP_WGRAD", "0"),)), "four launches")
    same_bits(four, trajectory(1, torch.bfloat16, False), "four launches vs the grouped launch")
    acc = trajectory(1, torch.bfloat16, True, shapes=((5, 40),), accum=2)
    same_bits(acc, trajectory(1, torch.bfloat16, False, shapes=((5, 40),), accum=2), "accumulation of 2")
    assert acc["stats"][1] == 8


def test_composition_with_freezing_layerwise_groups_and_clipping():
    """j = 2 with the embeddings and layers 0 - 1 frozen (everything below the gate), layer-wise groups and max_grad_norm = 1.0 in one
    trajectory: the input-gradient chain still runs through the frozen layers; only their weight gradients and updates are left out"""
    kw = dict(freeze=(True, (0, 1)), groups="classed", max_norm=1.0)
    ref = trajectory(2, torch.bfloat16, False, **kw)
    graph = trajectory(2, torch.bfloat16, True, **kw)
    same_bits(graph, ref, "graph")
    for run, what in ((graph, "graph"), (ref, "unfused")):
        frozen_untouched(run, what)
    accounted(graph)
    elems = int(graph["mask"][: graph["n"]].sum())
    assert graph["frozen"] == [(elems, 2, 1)] * 4, graph["frozen"]


# ------------------------------------------------------------------------------------------------------ 9: optimizer trajectory
def test_three_optimizer_steps_track_the_oracle_fp32():
    j, layers = 1, 2
    m = make(j, layers=layers).train()
    o = oracle(j, layers=layers).train()
    opt = AdamW(optimizer_grouped_parameters(m), lr=1e-3)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    oo = O.AdamW(O.grouped_parameters(o), lr=1e-3)
    so = O.get_linear_schedule_with_warmup(oo, num_warmup_steps=1.0, num_training_steps=10)
    for s in range(3):
        b = weights.synthetic_bert_batch(4, 50, 47, A_DIM, seed=50 + s)
        m.training_step(*tb(b, DEV))
        opt.step(); sch.step(); opt.zero_grad()
        oo.zero_grad()
        mse_backward(o, tb(b))
        oo.step(); so.step()
    torch.cuda.synchronize()
    assert float(m.flat_grads.abs().max()) == 0.0
    om = dict(o.named_parameters())
    worst = max(float((p.detach().cpu() - om[n].detach()).abs().max()) for n, p in m.named_parameters())
    print("j=1 max |param - oracle param| after 3 steps:", worst)
    assert worst <= 2e-4
    m.eval(); o.eval()
    b = weights.synthetic_bert_batch(4, 50, 47, A_DIM, seed=60)
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    i2, v2, a2, m2, s2, _ = tb(b)
    with torch.no_grad():
        d = float((m(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].cpu() - o(i2, v2, a2, m2, s2)[0]).abs().max())
    assert d <= 5e-3


# ------------------------------------------------------------------------------------------------------------ 10: data parallel
# test_dp_gpu's engine worker with the model class bound to an injection index (its `build` is test_model_gpu's)
_DP_WORKER = r'''
import functools, os, sys
sys.path.insert(0, os.environ["REPO_ROOT"]); sys.path.insert(0, os.path.join(os.environ["REPO_ROOT"], "tests"))
import test_model_gpu as T
T.MAG_BertForSequenceClassification = functools.partial(T.MAG_BertForSequenceClassification, injection_index=int(os.environ["INJECT"]))
''' + _ENGINE_WORKER


def _dp_run(tmp_path, world, env_extra, tag):
    script = tmp_path / (tag + ".py")
    script.write_text(_DP_WORKER)
    port = free_port()
    procs = []
    for r in range(world):
        e = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), REPO_ROOT=ROOT,
                 HSA_ENABLE_IPC_MODE_LEGACY="0", KIND="bert", **env_extra)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out.decode()[-3000:]


def test_single_call_dp_step_one_rank_rccl_and_two_callback_ranks(tmp_path):
    """j = 1, fp32, dropout off, deterministic mode, three steps: the single-call data-parallel step over a one-rank RCCL communicator ends
    on the bits of the plain single-call step (test_dp_gpu.test_single_call_dp_step_over_rccl_one_rank); two callback ranks with half the
    batch each deliver its first moment to 5e-6 and stay in lock-step (test_single_call_dp_step_two_ranks_equal_one_process)"""
    out = str(tmp_path / "dp")
    common = dict(OUT=out, INJECT="1", STEPS="3", CDT="fp32", MB_DETERMINISTIC="1")
    _dp_run(tmp_path, 1, dict(common, USE_DP="0"), "one")
    _dp_run(tmp_path, 1, dict(common, USE_DP="1", MB_DP_FORCE="1", BACKEND="nccl", MB_DP_GRAD_DTYPE="fp32"), "rccl")
    ref, one = torch.load(out + ".1.0.0"), torch.load(out + ".1.0.1")
    assert one["fused"] and not ref["fused"]
    assert torch.equal(ref["p"], one["p"])
    _dp_run(tmp_path, 2, dict(common, USE_DP="1", MB_DP_SPARSE_EMB="1", MB_DP_CHUNK="2"), "two")
    a, b = torch.load(out + ".2.0.1"), torch.load(out + ".2.1.1")
    assert a["fused"] and b["fused"] and a["sparse"]
    assert torch.equal(a["p"], b["p"]) and torch.equal(a["m"], b["m"])
    err = float((a["m"] - ref["m"]).abs().max()) / float(ref["m"].abs().max())
    print("j=1 single-call DP(2 x 4) vs single(8): first-moment max |d| / max = %.3e" % err)
    assert err <= 5e-6
    assert float((a["p"] - ref["p"]).abs().max()) <= 3 * 1e-3 * 1.1          # three updates of at most lr each


def test_sharded_step_with_a_cut_forward_and_the_gate_behind_the_first_seam(tmp_path):
    """4 layers, one per piece, j = 2: the forward is cut into four graphs and the gate runs in the third (test_dp_gpu.
    test_sharded_step_with_a_cut_forward_over_rccl_one_rank): bit-identical to the plain single-call step after three steps"""
    out = str(tmp_path / "cut")
    common = dict(OUT=out, INJECT="2", MB_DP_FORCE="1", BACKEND="nccl", STEPS="3", CDT="bf16", MB_DETERMINISTIC="1", LAYERS="4", MB_DP_CHUNK="1",
                  MB_DP_GRAD_DTYPE="fp32")
    _dp_run(tmp_path, 1, dict(common, USE_DP="0"), "plain")
    _dp_run(tmp_path, 1, dict(common, USE_DP="1", MB_DP_SHARD_OPT="1", MB_DP_SHARD_FORCE="1"), "cut")
    a, b = torch.load(out + ".1.0.0"), torch.load(out + ".1.0.1")
    assert b["fused"] and not a["fused"] and b["slices"] and len(b["slices"]) == 3
    assert torch.equal(a["p"], b["p"])


# ------------------------------------------------------------------------------------------------- 11: j = 0 and the driver
def test_index_zero_is_the_model_built_without_the_argument():
    b = weights.synthetic_bert_batch(4, 50, 47, A_DIM, seed=21)
    outs = []
    for j in (None, 0):
        with env(MB_DETERMINISTIC=1):          # (the column sums of a plain run are atomics: their bits vary from run to run)
            m = make(j, torch.bfloat16, layers=2).train()
            assert m._core.injection_index == 0
            m.eval()
            ids, vis, aco, mask, seg, lab = tb(b, DEV)
            with torch.no_grad():
                logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].clone()
            m.train()
            m.training_step(ids, vis, aco, mask, seg, lab)
            torch.cuda.synchronize()
            outs.append((logits, m.flat_grads.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    same_bits(trajectory(0, torch.bfloat16, True, nsteps=2), trajectory(None, torch.bfloat16, True, nsteps=2), "j = 0")
    with pytest.raises(ValueError) as ei:
        make(3, layers=3)
    assert "injection_index" in str(ei.value) and "num_hidden_layers" in str(ei.value)


def test_engine_is_recreated_with_its_index():
    """a larger batch re-creates the engine (_Core._make_engine): the gate stays where the constructor put it"""
    m = make(1, kw=SMALL_KW, p_mag=0.5).eval()
    o = oracle(1, kw=SMALL_KW, p_mag=0.5).eval()
    for (B, L) in ((2, 8), (6, 60)):
        b = weights.synthetic_bert_batch(B, L, 47, A_DIM, seed=3)
        ids, vis, aco, mask, seg, _ = tb(b, DEV)
        i2, v2, a2, m2, s2, _ = tb(b)
        with torch.no_grad():
            assert float((m(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].cpu() - o(i2, v2, a2, m2, s2)[0]).abs().max()) <= 1e-3
    assert m._core.max_B >= 6 and m._core.max_L >= 60


@pytest.mark.parametrize("model,inj", [("bert-base-uncased", "1"), ("xlnet-base-cased", "2")])
def test_driver_epochs_run_and_learn(model, inj, monkeypatch, capsys):
    """--synthetic 192 --injection_index N with the model's configuration cut to 3 layers: finite, decreasing training loss"""
    from bert_multimodal_transformer_amd import multimodal_driver as D
    seen = {}
    monkeypatch.setattr(D, "bert_config", lambda model, num_labels=1: BertConfig(num_hidden_layers=3, num_labels=num_labels))
    monkeypatch.setattr(D, "xlnet_config", lambda model, num_labels=1: XLNetConfig(n_layer=3, num_labels=num_labels))
    prep = D.prep_for_training

    def spy(n):
        r = prep(n)
        seen["index"] = r[0]._core.injection_index
        return r

    monkeypatch.setattr(D, "prep_for_training", spy)
    old = getattr(D, "args", None)
    try:
        D.main(["--model", model, "--synthetic", "192", "--n_epochs", "4", "--seed", "5", "--learning_rate", "5e-5", "--injection_index", inj])
    finally:
        D.args = old
    recs = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    losses = [r["train_loss"] for r in recs if "train_loss" in r]
    print("%s --injection_index %s: epoch losses %s" % (model, inj, losses))
    assert seen["index"] == int(inj)
    assert len(losses) == 4 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
