"""GPU: MAG-XLNet at the widths next to xlnet-base -- d_model 256 (4 heads), 512 (8 heads) and 1024 (16 heads, xlnet-large-cased).

References: tests/golden/g12_xlnet_sizes.npz (the reference's own logits at full depth, one mems and one query-stream case at 2 x 1024:
scripts/make_golden_xlnet_sizes.py) and the CPU oracle run live on the same inputs.  Bounds are the 768 tests': fp32 logits 1e-3, fp32
gradients 5e-3 of the tensor's max, bf16 at 2 layers logits 1e-2 / gradients 3e-2 relative Frobenius (MAG's gated tensors 1e-1); at full
depth the bf16 logit bound is 5e-2 -- the bound of test_xlnet_gpu.test_eval_logits_bf16 at 12 x 768 -- scaled by the oracle's own
bf16-autocast error at the new size over its autocast error at 12 x 768 on the same batch (never below 5e-2), both computed live.
Oracles are built once per (width, depth, visual width) and shared; only the optimizer test, which moves the weights, builds its own."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, MAG_XLNetForSequenceClassification, MAG_XLNetModel, MultimodalConfig, XLNetConfig,
                                             _lib, get_linear_schedule_with_warmup)
from oracle import mag_xlnet_ref as X, optim_ref as O, weights
from test_bert_sizes_gpu import _same
from test_xlnet_gpu import DEV, LOOSE_BF16, _grad_report, tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_xlnet_sizes import CASES, EXTRA_H, EXTRA_LAYERS, MEMS_CASE, QS_CASE, SAMPLE, SIZES, key, query_stream_inputs, size_config      # noqa: E402

NEW = [s[0] for s in SIZES]          # 1024, 512, 256


@functools.lru_cache(maxsize=None)
def _param(name, shape):
    """oracle/weights.py's "test" value of one tensor, generated once per process (a 24 x 1024 model is 360 M hashed values)"""
    return torch.from_numpy(weights.make_param(name, shape, "test"))


def make(H, layers=None, cdt=torch.float32, V=47, p_mag=0.0, p=0.0, mem_len=None, max_seq_length=None):
    cfg = XLNetConfig(dropout=p, summary_last_dropout=p, mem_len=mem_len, **size_config(H, layers))
    m = MAG_XLNetForSequenceClassification(cfg, MultimodalConfig(1.0, p_mag), visual_dim=V, acoustic_dim=74, compute_dtype=cdt,
                                           max_seq_length=max_seq_length)
    m.load_state_dict({n: _param(n, tuple(q.shape)) for n, q in m.named_parameters()})
    return m


def fresh_oracle(H, layers=None, V=47):
    kw = size_config(H, layers) if H != 768 else dict(n_layer=12 if layers is None else layers)
    o = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**kw), X.MultimodalConfig(1.0, 0.0), V, 74)
    with torch.no_grad():                      # (X.load_deterministic(o, "test") through the cache)
        for n, q in o.named_parameters():
            q.copy_(_param(n, tuple(q.shape)))
    return X.set_dropout(o, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def _shared_oracle(H, layers, V):
    return fresh_oracle(H, layers, V)


def oracle(H, layers=None, V=47):
    """the shared oracle of this size, every dropout p = 0, gradients cleared (its weights are never changed)"""
    o = _shared_oracle(H, layers, V)
    o.zero_grad(set_to_none=True)
    return o


def eval_logits(m, b, **kw):
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    with torch.no_grad():
        return m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, **kw)[0].float().cpu()


def oracle_logits(o, b, **kw):
    i2, v2, a2, m2, s2, _ = tb(b)
    with torch.no_grad():
        return o(i2, v2, a2, m2, s2, **kw)[0]


def _train_pair(m, o, b, **kw):
    """one forward + MSE + backward on both sides (train mode, p = 0) -> (logits, oracle logits)"""
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    out = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None, **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()})
    torch.nn.MSELoss()(out[0].view(-1), lab.view(-1)).backward()
    i2, v2, a2, m2, s2, l2 = tb(b)
    lo = o(i2, v2, a2, m2, s2, **{k: v for k, v in kw.items() if k != "output_attentions"})[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    return out, lo


# ------------------------------------------------------------------------------------------------------------ 1. fp32 parity, full depth
@pytest.mark.parametrize("B,L,V,seed", CASES)
@pytest.mark.parametrize("H", NEW)
def test_fp32_logits_vs_reference_fixture_and_oracle(golden, H, B, L, V, seed):
    """full depth (24 x 1024, 8 x 512, 4 x 256), eval: the project's contract, |logit error| <= 1e-3"""
    g = golden["g12_xlnet_sizes"]
    m = make(H, None, torch.float32, V, p_mag=0.5, p=0.1).eval()
    b = weights.synthetic_xlnet_batch(B, L, V, 74, seed=seed)
    got = eval_logits(m, b)
    seq = m._core.sequence_output(B, L).float().cpu().numpy()
    err = float(np.abs(got.numpy() - g[key("logits", H, B, L, V, seed)]).max())
    err_seq = float(np.abs(weights.strided_sample(seq, SAMPLE) - g[key("seq", H, B, L, V, seed)]).max())
    live = float((got - oracle_logits(oracle(H, None, V).eval(), b)).abs().max())
    print("fp32 H=%d B=%d L=%d V=%d: logits max|err| vs fixture %.3e, vs live oracle %.3e; transformer output sample %.3e" % (H, B, L, V, err, live, err_seq))
    assert err <= 1e-3 and live <= 1e-3 and err_seq <= 1e-3


# ------------------------------------------------------------------------------------------------------------ 2. fp32 gradients
@pytest.mark.parametrize("H,layers", [(256, 2), (512, 2), (1024, 2), (1024, None)])
def test_fp32_gradients_vs_oracle(H, layers):
    """train mode, every dropout p = 0: loss and ALL parameter gradients, 2 layers at each new width and xlnet-large at full depth"""
    m = make(H, layers, torch.float32).train()
    o = oracle(H, layers).train()
    b = weights.synthetic_xlnet_batch(4, 50, 47, 74, seed=21)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    out, lo = _train_pair(m, o, b)
    loss = float(torch.nn.MSELoss()(out[0].detach().view(-1), lab.view(-1)))
    loss_o = float(F.mse_loss(lo.detach().view(-1), tb(b)[5].view(-1)))
    print("fp32 H=%d layers=%s: loss %.6f oracle %.6f" % (H, layers, loss, loss_o))
    assert abs(loss - loss_o) < 1e-4
    _grad_report(m, o, 5e-3, show=3)
    # the fused step gives the same gradients (its loss lives inside the head kernel)
    g_ref = m.flat_grads.clone()
    m.zero_grad()
    l2_ = m.training_step(ids, vis, aco, mask, seg, lab)
    assert abs(float(l2_) - loss) < 1e-5
    assert float((m.flat_grads - g_ref).abs().max()) <= 1e-5 * float(g_ref.abs().max()) + 1e-9


# ------------------------------------------------------------------------------------------------------------ 3. ragged shapes
@pytest.mark.parametrize("B,L", [(3, 17), (5, 33), (2, 65), (1, 97), (2, 128)])
@pytest.mark.parametrize("H", [1024, 256])
def test_ragged_shapes_eval_fp32(H, B, L):
    """odd B x 16 (4) heads and every LP bucket of the LDS-resident kernels (32, 64, 128), lengths that are no multiple of 16, one row
    without padding"""
    m = make(H, 2, p_mag=0.5, p=0.1).eval()
    o = oracle(H, 2).eval()
    b = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=70 + L)
    b["input_mask"][0, :] = 1
    err = float((eval_logits(m, b) - oracle_logits(o, b)).abs().max())
    print("H=%d B=%d L=%d max|err| %.3e" % (H, B, L, err))
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------------------ 4. long sequences
def test_long_sequences_at_1024():
    """max_seq_length = 256 at 16 heads: L = 200 (the tiled relative attention, per-layer row statistics) and L = 40 on the same engine
    (the LDS-resident kernels with the 128-row psave a tiled engine keeps per layer), train mode (p = 0), fp32, against the oracle with
    the bounds of the longest fp32 case of test_xlnet_gpu.test_long_sequences_train_vs_oracle: logits 1e-3, probabilities 1e-5,
    gradients 1e-2 of the tensor's max.  L = 257 raises."""
    H, layers, nh = 1024, 2, 16
    m = make(H, layers, torch.float32, max_seq_length=256).train()
    o = oracle(H, layers).train()
    for (B, L) in ((2, 200), (3, 40)):
        b = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=90 + L)
        b["input_mask"][0, :] = 1                                    # one row without padding: every key beyond 128 is live
        m.zero_grad(); o.zero_grad(set_to_none=True)
        out, lo = _train_pair(m, o, b, output_attentions=True)
        logits, att = out[0], out[1]
        err = float((logits.detach().cpu() - lo.detach()).abs().max())
        perr = max(float((att[l].cpu() - lyr.rel_attn.last_probs.detach()).abs().max()) for l, lyr in enumerate(o.transformer.layer))
        print("H=1024 max_seq_length=256, L=%d: logits %.2e, probabilities %.2e" % (L, err, perr))
        assert tuple(att[0].shape) == (B, nh, L, L)
        assert err <= 1e-3 and perr <= 1e-5
        _grad_report(m, o, 1e-2, show=2)
        m.zero_grad()
        m.train_step(*tb(b, DEV), optimizer=None)                  # the single-call step at this length (graph capture included)
        torch.cuda.synchronize()
    with pytest.raises(_lib.MagbertError):
        eval_logits(m, weights.synthetic_xlnet_batch(2, 257, 47, 74, seed=1))


# ------------------------------------------------------------------------------------------------------------ 5. optional arguments
def _oracle_hidden(o, run):
    """the oracle's hidden states as [B, L, H]: the input of layer 0, then every layer's output"""
    hooks, ref_h = [], []
    hooks.append(o.transformer.layer[0].register_forward_pre_hook(lambda mod, args: ref_h.append(args[0].detach())))
    for lyr in o.transformer.layer:
        hooks.append(lyr.register_forward_hook(lambda mod, args, out: ref_h.append(out.detach())))
    try:
        r = run()
    finally:
        for h in hooks:
            h.remove()
    return r, [h.permute(1, 0, 2) for h in ref_h]


def test_hidden_states_attentions_head_mask_and_masks_at_1024():
    """output_hidden_states / output_attentions ([B, 16, L, L]; 1e-3 and 1e-4), head_mask with the last of the 16 heads at 0.5 and another
    at 0, perm_mask + input_mask -- eval, fp32, 2 layers, against the oracle"""
    H, layers, nh, B, L = 1024, 2, 16, 3, 40
    m = make(H, layers, p_mag=0.5, p=0.1).eval()
    o = oracle(H, layers).eval()
    b = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=83)
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    with torch.no_grad():
        got = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, output_hidden_states=True, output_attentions=True)
        base = m.transformer(ids, vis, aco, token_type_ids=seg, attention_mask=mask, output_attentions=True)
    ref, ref_h = _oracle_hidden(o, lambda: oracle_logits(o, b))
    logits, hs, att = got
    assert float((logits.cpu() - ref).abs().max()) <= 1e-3
    assert len(hs) == layers + 1 and tuple(hs[0].shape) == (B, L, H) and len(ref_h) == layers + 1
    for h, r in zip(hs, ref_h):
        assert float((h.cpu() - r).abs().max()) <= 1e-3
    assert len(att) == layers and tuple(att[0].shape) == (B, nh, L, L)
    for a, lyr in zip(att, o.transformer.layer):
        assert float((a.cpu() - lyr.rel_attn.last_probs).abs().max()) <= 1e-4
        assert float((a.sum(-1) - 1.0).abs().max()) <= 1e-4
    assert len(base) == 2 and float((base[1][0] - att[0]).abs().max()) == 0.0
    hm = torch.ones(layers, nh)
    hm[0, 2] = 0.0
    hm[1, 15] = 0.5                               # the last of the 16 heads
    with torch.no_grad():
        out = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, head_mask=hm.to(DEV), output_attentions=True)
    r = oracle_logits(o, b, head_mask=hm)
    assert float((out[0].cpu() - r).abs().max()) <= 1e-3 and float((r - ref).abs().max()) > 1e-5
    assert float(out[1][0][:, 2].abs().max()) == 0.0
    assert float((out[1][1].cpu() - o.transformer.layer[1].rel_attn.last_probs).abs().max()) <= 1e-4
    # perm_mask + input_mask (1 = padding) in place of attention_mask
    perm = torch.from_numpy((np.random.RandomState(77).rand(B, L, L) < 0.3).astype(np.float32))
    im = 1.0 - mask.float()
    with torch.no_grad():
        a = m(ids, vis, aco, token_type_ids=seg, input_mask=im, perm_mask=perm.to(DEV))[0].cpu()
        plain = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].cpu()
        i2, v2, a2, m2, s2, _ = tb(b)
        want = o(i2, v2, a2, None, s2, perm_mask=perm, input_mask=1.0 - m2.float())[0]
    e = float((a - want).abs().max())
    print("H=1024 perm_mask + input_mask: logits %.2e (the masks move them by %.2e)" % (e, float((want - ref).abs().max())))
    assert e <= 1e-3 and float((want - ref).abs().max()) > 1e-4 and float((plain - ref).abs().max()) <= 1e-3


def test_inputs_embeds_and_trainable_base_model_at_1024():
    """inputs_embeds with its gradient (logits 1e-3, d(inputs_embeds) 2e-3 relative Frobenius, parameters 5e-3), and the differentiable
    base model: a head on MAG_XLNetModel's output trains the whole stack (output 1e-3, gradients 5e-3) -- the bounds of
    test_xlnet_gpu.test_inputs_embeds_and_trainable_base_model_fp32"""
    H, layers, B, L = 1024, 2, 3, 24
    m = make(H, layers).train()
    o = oracle(H, layers).train()
    b = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=83)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    i2, v2, a2, m2, s2, l2 = tb(b)
    emb_cpu = (o.transformer.word_embedding(i2).detach() + 0.05 * torch.from_numpy(weights.make_param("probe.emb", (B, L, H), "test"))).requires_grad_(True)
    emb = emb_cpu.detach().to(DEV).requires_grad_(True)
    logits = m(None, vis, aco, attention_mask=mask, token_type_ids=seg, inputs_embeds=emb)[0]
    torch.nn.MSELoss()(logits.view(-1), lab.view(-1)).backward()
    lo = o(None, v2, a2, m2, s2, inputs_embeds=emb_cpu)[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu() - lo.detach()).abs().max())
    gerr = float((emb.grad.cpu() - emb_cpu.grad).norm() / emb_cpu.grad.norm())
    print("H=1024 inputs_embeds: logits %.2e, d(inputs_embeds) rel. Frobenius %.2e" % (err, gerr))
    assert err <= 1e-3 and gerr <= 2e-3
    word = dict(m.named_parameters())["transformer.word_embedding.weight"]
    assert float(word.grad.abs().max()) == 0.0 and o.transformer.word_embedding.weight.grad is None
    o.transformer.word_embedding.weight.grad = torch.zeros_like(o.transformer.word_embedding.weight)
    _grad_report(m, o, 5e-3)
    o.zero_grad(set_to_none=True)
    # the base model: a head on its output back-propagates into the engine
    cfg = XLNetConfig(dropout=0.0, summary_last_dropout=0.0, **size_config(H, layers))
    base = MAG_XLNetModel(cfg, MultimodalConfig(1.0, 0.0), 47, 74).train()
    base.load_state_dict({n: _param("transformer." + n, tuple(q.shape)) for n, q in base.named_parameters()})
    ob = o.transformer
    out = base(ids, vis, aco, attention_mask=mask, token_type_ids=seg)[0]
    assert out.requires_grad and tuple(out.shape) == (B, L, H)
    w = torch.from_numpy(weights.make_param("probe.seq", (H,), "test"))
    ((out * w.to(DEV)).sum(-1) ** 2).mean().backward()
    ro = ob(i2, v2, a2, m2, s2)
    ((ro * w).sum(-1) ** 2).mean().backward()
    torch.cuda.synchronize()
    assert float((out.detach().cpu() - ro.detach()).abs().max()) <= 1e-3
    og = {n: q.grad for n, q in ob.named_parameters() if q.grad is not None}
    gmax = max(float(g.abs().max()) for g in og.values())
    rows = sorted(((float((q.grad.cpu() - og[n]).abs().max()) / max(float(og[n].abs().max()), 1e-3 * gmax), n)
                   for n, q in base.named_parameters() if n in og), reverse=True)
    print("H=1024 base-model gradients through the autograd edge: worst relative errors", ["%.2e %s" % r for r in rows[:4]])
    assert rows[0][0] <= 5e-3


# ------------------------------------------------------------------------------------------------------------ 6. mems
def test_mems_match_reference_fixture_at_1024(golden):
    """segment 1 caches (use_cache, mem_len 40), segment 2 consumes the cache (klen = 90) and caches again: logits of both segments and
    samples of the cached memories against the REFERENCE's values, fp32 <= 1e-3; new_mems are (min(mem_len, ...), B, 1024)"""
    H = EXTRA_H
    B, L, ml, seed = MEMS_CASE
    g = golden["g12_xlnet_sizes"]
    tag = "H%d/B%d_L%d_M%d_seed%d" % (H, B, L, ml, seed)
    m = make(H, EXTRA_LAYERS, p_mag=0.5, p=0.1, mem_len=ml).eval()
    o = oracle(H, EXTRA_LAYERS).eval()
    b1, b2 = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed), weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed + 100)
    i1, v1, a1, m1, s1, _ = tb(b1, DEV)
    i2, v2, a2, m2, s2, _ = tb(b2, DEV)
    with torch.no_grad():
        r1 = m(i1, v1, a1, token_type_ids=s1, attention_mask=m1, use_cache=True)
        assert len(r1) == 2 and len(r1[1]) == EXTRA_LAYERS and tuple(r1[1][0].shape) == (min(ml, L), B, H)
        r2 = m(i2, v2, a2, token_type_ids=s2, attention_mask=m2, use_cache=True, mems=list(r1[1]), output_attentions=True)
        lo = oracle_logits(o, b2, mems=[t.cpu() for t in r1[1]], mem_len=ml)
    e1 = float(np.abs(r1[0].cpu().numpy() - g["mems/logits_seg1/" + tag]).max())
    e2 = float(np.abs(r2[0].cpu().numpy() - g["mems/logits_seg2/" + tag]).max())
    eo = float((r2[0].cpu() - lo).abs().max())
    print("H=1024 mems %s: logits vs the fixture seg 1 %.2e, seg 2 %.2e (vs the oracle fed OUR memories %.2e)" % (tag, e1, e2, eo))
    assert e1 <= 1e-3 and e2 <= 1e-3 and eo <= 1e-3
    assert len(r2) == 3 and tuple(r2[1][0].shape) == (min(ml, 2 * L), B, H)
    worst = 0.0
    for name, mems in (("seg1", r1[1]), ("seg2", r2[1])):
        for i in range(EXTRA_LAYERS):
            ref = g["mems/new_mems_%s/%s/layer%d" % (name, tag, i)]
            got = weights.strided_sample(mems[i].float().cpu().numpy(), SAMPLE)
            worst = max(worst, float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-6))
    assert worst <= 1e-3
    assert tuple(r2[2][0].shape) == (B, 16, L, min(ml, L) + L)
    perr = max(float((r2[2][l].cpu() - lyr.rel_attn.last_probs).abs().max()) for l, lyr in enumerate(o.transformer.layer))
    assert perr <= 1e-5


def test_mems_training_gradients_vs_oracle_at_1024():
    """training with cached (detached) memories, klen = 90: logits 1e-3 and every parameter gradient within 5e-3 of the oracle's -- the
    tolerance of test_xlnet_gpu.test_mems_training_gradients_vs_oracle in fp32"""
    H, layers = 1024, 2
    B, L, ml, _ = MEMS_CASE
    m = make(H, layers).train()
    o = oracle(H, layers).train()
    b = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=91)
    gen = torch.Generator().manual_seed(5)
    mems = [torch.randn(ml, B, H, generator=gen) * 0.5 for _ in range(layers)]
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, mems=[t.to(DEV) for t in mems], labels=None)[0]
    torch.nn.MSELoss()(logits.view(-1), lab.view(-1)).backward()
    i2, v2, a2, m2, s2, l2 = tb(b)
    lo = o(i2, v2, a2, m2, s2, mems=mems)[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu() - lo.detach()).abs().max())
    print("H=1024 mems training (klen %d): logits %.2e" % (ml + L, err))
    assert err <= 1e-3
    _grad_report(m, o, 5e-3, show=3)
    m.zero_grad()
    m.train_step(ids, vis, aco, mask, seg, lab, optimizer=None)          # the plain pass afterwards is unaffected
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ 7. query stream
def test_query_stream_matches_reference_fixture_at_1024(golden):
    """target_mapping at 16 heads: output_g [B, M, 1024] and the classifier's logits on it against the REFERENCE's values (fixture) and the
    oracle run live, fp32 <= 1e-3 (the bounds of test_xlnet_gpu.test_query_stream_matches_reference_golden)"""
    H = EXTRA_H
    B, L, M, seed = QS_CASE
    g = golden["g12_xlnet_sizes"]
    tag = "H%d/B%d_L%d_M%d_seed%d" % (H, B, L, M, seed)
    m = make(H, EXTRA_LAYERS, p_mag=0.5, p=0.1).eval()
    o = oracle(H, EXTRA_LAYERS).eval()
    b = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed)
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    tm, pm = query_stream_inputs(b["input_mask"], M, seed)
    tm_t, pm_t = torch.from_numpy(tm), torch.from_numpy(pm)
    with torch.no_grad():
        plain = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t.to(DEV))[0].cpu().numpy()
        r = m.transformer(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t.to(DEV), target_mapping=tm_t.to(DEV),
                          output_hidden_states=True)
        logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t.to(DEV), target_mapping=tm_t.to(DEV))[0].cpu().numpy()
        again = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t.to(DEV))[0].cpu().numpy()
        c = tb(b)
        want_g = o.transformer(c[0], c[1], c[2], c[3], c[4], perm_mask=pm_t, target_mapping=tm_t)
        want_l = o(c[0], c[1], c[2], c[3], c[4], perm_mask=pm_t, target_mapping=tm_t)[0]
    out_g = r[0].cpu()
    e_g = float(np.abs(weights.strided_sample(out_g.numpy(), SAMPLE) - g["qs/output_g/" + tag]).max())
    e_l = float(np.abs(logits - g["qs/logits/" + tag]).max())
    e_go, e_lo = float((out_g - want_g).abs().max()), float(np.abs(logits - want_l.numpy()).max())
    print("H=1024 query stream %s: output_g err %.2e (fixture sample) %.2e (oracle, |g| max %.2f), logits err %.2e / %.2e"
          % (tag, e_g, e_go, float(want_g.abs().max()), e_l, e_lo))
    assert tuple(out_g.shape) == (B, M, H) and max(e_g, e_go) <= 1e-3 and max(e_l, e_lo) <= 1e-3
    assert np.array_equal(plain, again)                       # the post-pass leaves nothing behind in the engine
    hs = r[1]
    assert len(hs) == 2 * (EXTRA_LAYERS + 1) and tuple(hs[0].shape) == (B, L, H) and tuple(hs[1].shape) == (B, M, H)
    assert float((hs[1] - m.transformer.mask_emb.detach().float().view(1, 1, H)).abs().max()) == 0.0
    assert float((hs[-1] - r[0]).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 8. / 9. bf16
@pytest.mark.parametrize("H", NEW)
def test_bf16_two_layers_vs_oracle(H):
    """the 768 tests' bf16 bounds at 2 layers: logits 1e-2, gradients 3e-2 relative Frobenius, MAG's gated tensors 1e-1"""
    m = make(H, 2, torch.bfloat16).train()
    o = oracle(H, 2).train()
    b = weights.synthetic_xlnet_batch(4, 50, 47, 74, seed=21)
    out, lo = _train_pair(m, o, b)
    err = float((out[0].detach().float().cpu() - lo.detach()).abs().max())
    print("bf16 H=%d 2 layers: logits max|err| %.3e" % (H, err))
    assert err <= 1e-2
    _grad_report(m, o, 3e-2, frobenius=True, loose=LOOSE_BF16, tol_loose=1e-1, show=4)


def _autocast_error(o, b):
    i2, v2, a2, m2, s2, _ = tb(b)
    with torch.no_grad():
        exact = o(i2, v2, a2, m2, s2)[0]
        with torch.autocast("cpu", torch.bfloat16):
            low = o(i2, v2, a2, m2, s2)[0]
    return float((low.float() - exact).abs().max())


@pytest.mark.parametrize("H", NEW)
def test_bf16_full_depth_logits(golden, H):
    """bound = 5e-2 (the bound of test_xlnet_gpu.test_eval_logits_bf16 at 12 x 768) x max(1, a / b): a = the fp32 oracle's bf16-autocast
    error at this size and full depth, b = its autocast error at 12 x 768, same batch -- a ratio that comes from the oracle alone"""
    B, L, V, seed = CASES[0]
    b = weights.synthetic_xlnet_batch(B, L, V, 74, seed=seed)
    a_err = _autocast_error(oracle(H, None, V).eval(), b)
    b_err = _autocast_error(oracle(768, None, V).eval(), b)
    bound = 5e-2 * max(1.0, a_err / b_err)
    m = make(H, None, torch.bfloat16, V, p_mag=0.5, p=0.1).eval()
    got = eval_logits(m, b)
    err = float(np.abs(got.numpy() - golden["g12_xlnet_sizes"][key("logits", H, B, L, V, seed)]).max())
    print("bf16 H=%d full depth: logits max|err| %.3e ; oracle autocast error %.3e at this size, %.3e at 12 x 768 -> bound %.3e" % (H, err, a_err, b_err, bound))
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------ 10. / 11. the single-call step
def _steps(H, layers, cdt, graph, shapes=((4, 50),), nsteps=3, lr=1e-3, p=0.0, p_mag=0.0, seed0=50):
    from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
    torch.manual_seed(77)
    m = make(H, layers, cdt, p=p, p_mag=p_mag).train()
    opt = AdamW(optimizer_grouped_parameters(m), lr=lr)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    losses, batches = [], []
    with m.stream_scope():
        for s in range(nsteps):
            B, L = shapes[s % len(shapes)]
            batches.append(weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed0 + s))
            m.train_step(*tb(batches[-1], DEV), optimizer=opt, graph=graph)
            losses.append(m._core.loss_buf[0].clone())
            sch.step()
    torch.cuda.synchronize()
    core = m._core
    out = dict(model=m, opt=opt, sch=sch, losses=[float(x) for x in losses], batches=batches, stats=core.graph_stats(),
               frozen=m.transformer.mask_emb.detach().clone())
    if nsteps:
        out.update(p=m.flat_params.clone(), m=core._adam_m.clone(), v=core._adam_v.clone(), shadow=core.shadow.clone(), g=m.flat_grads.clone())
    return out


def test_three_single_call_steps_track_the_oracle_at_1024_fp32():
    """train_step(graph=True) at d_model = 1024: fwd + bwd + fused HF-AdamW + linear warmup, 3 steps, dropout off, against the oracle +
    optim_ref with the bounds of test_xlnet_gpu.test_three_optimizer_steps_track_the_oracle_fp32 (parameters 2e-4, eval logits 5e-3)"""
    H, layers = 1024, 2
    mask0 = _param("transformer.mask_emb", (1, 1, H))
    run = _steps(H, layers, torch.float32, True)
    m = run["model"]
    assert run["stats"][0] >= 1 and run["stats"][1] == 3
    o = fresh_oracle(H, layers).train()          # (its weights move: not the shared one)
    oo = O.AdamW(O.grouped_parameters(o), lr=1e-3)
    so = O.get_linear_schedule_with_warmup(oo, num_warmup_steps=1.0, num_training_steps=10)
    ref = []
    for b in run["batches"]:
        i2, v2, a2, m2, s2, l2 = tb(b)
        oo.zero_grad()
        loss = F.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1))
        ref.append(float(loss.detach()))
        loss.backward()
        oo.step(); so.step()
    assert float(m.flat_grads.abs().max()) == 0.0
    assert torch.equal(run["frozen"].cpu(), mask0)                     # no gradient -> HF AdamW never touches it
    om = dict(o.named_parameters())
    worst = max(float((p.detach().cpu() - om[n].detach()).abs().max()) for n, p in m.named_parameters())
    print("H=1024 single-call steps: losses %s oracle %s ; max |param - oracle param| %.3e" % (run["losses"], ref, worst))
    for a, r in zip(run["losses"], ref):
        assert abs(a - r) <= 1e-3 * max(1.0, abs(r))
    assert worst <= 2e-4
    m.eval(); o.eval()
    b = weights.synthetic_xlnet_batch(4, 50, 47, 74, seed=60)
    assert float((eval_logits(m, b) - oracle_logits(o, b)).abs().max()) <= 5e-3


def test_graph_step_equals_launch_by_launch_at_1024(monkeypatch):
    """deterministic mode, bf16, dropout on, two shapes: the replayed graph ends every step with the bits of the same launches one by one"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    kw = dict(shapes=((5, 50), (3, 40)), nsteps=4, p=0.1, p_mag=0.5)
    g = _steps(1024, 2, torch.bfloat16, True, **kw)
    e = _steps(1024, 2, torch.bfloat16, "launches", **kw)
    assert g["stats"] == (2, 4) and e["stats"] == (0, 0), (g["stats"], e["stats"])
    _same(g, e, "graph vs launches")
    assert torch.equal(g["frozen"], e["frozen"])
    assert max(abs(a - b) for a, b in zip(g["losses"], e["losses"])) <= 2e-3


@pytest.mark.parametrize("H,layers,shapes", [(256, 2, ((5, 40), (5, 40), (3, 24), (5, 40))), (1024, 2, ((5, 40), (5, 40), (3, 24), (5, 40))),
                                             (1024, None, ((2, 24),))])
def test_riders_change_nothing(monkeypatch, H, layers, shapes):
    """MB_ADAMW_RIDE in the MAG-XLNet engine at 4 and 16 heads (the pattern of test_xlnet_gpu.test_xlnet_adamw_riders_change_nothing):
    deterministic mode, bf16, dropout on, 4 steps -- parameters and both moments end with the SAME BITS with and without riders, the
    losses agree to rtol 1e-6, gradients read as zeros.  24 x 1024: the depth at which most of the update is final long before the
    backward ends, so what no launch carried is a large sweep."""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    kw = dict(shapes=shapes, nsteps=4, p=0.1, p_mag=0.5, seed0=90)
    monkeypatch.setenv("MB_ADAMW_RIDE", "0")
    ref = _steps(H, layers, torch.bfloat16, True, **kw)
    del ref["model"], ref["opt"], ref["sch"]
    torch.cuda.empty_cache()
    monkeypatch.delenv("MB_ADAMW_RIDE")
    ride = _steps(H, layers, torch.bfloat16, True, **kw)
    _same(ride, ref, "riders on vs off")
    assert torch.allclose(torch.tensor(ride["losses"]), torch.tensor(ref["losses"]), rtol=1e-6, atol=0.0)      # (the batch mean is a float atomic sum)
    assert torch.equal(ride["frozen"], ref["frozen"]) and ride["stats"] == ref["stats"]


# ------------------------------------------------------------------------------------------------------------ 12. / 13. child processes
_WORKER = r'''
import os, sys, torch
sys.path.insert(0, os.environ["REPO_ROOT"]); sys.path.insert(0, os.path.join(os.environ["REPO_ROOT"], "tests"))
import torch.distributed as dist
from test_xlnet_sizes_gpu import _steps, make, tb, weights, DEV
job = os.environ["JOB"]
if job == "det":
    r = _steps(1024, 2, torch.bfloat16, {"graph": True, "launches": "launches"}[os.environ["MODE"]], shapes=((5, 50),), nsteps=4, p=0.1, p_mag=0.5, seed0=70)
    torch.save({k: r[k].cpu() for k in ("p", "m", "v", "shadow", "g")}, os.environ["OUT"])
else:                                  # the one-rank RCCL data-parallel step (or the plain one), xlnet-large at full depth
    from bert_multimodal_transformer_amd import AdamW, get_linear_schedule_with_warmup
    from bert_multimodal_transformer_amd.distributed import DataParallel
    from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
    torch.cuda.set_device(0)
    use_dp = os.environ["USE_DP"] == "1"
    if use_dp:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    m = make(1024, None, torch.float32).train()
    opt = AdamW(optimizer_grouped_parameters(m), lr=1e-3)
    sch = get_linear_schedule_with_warmup(opt, 0, 100)
    dp = None
    if use_dp:
        dp = DataParallel(m, opt)
        dp.broadcast_parameters(0)
    with m.stream_scope():
        for s in range(3):
            m.train_step(*tb(weights.synthetic_xlnet_batch(2, 24, 47, 74, seed=90 + s), DEV), optimizer=opt, graph=None)
            sch.step()
    torch.cuda.synchronize()
    fused = bool(dp is not None and dp._last_fused)
    torch.save(dict(p=m.flat_params.cpu(), fused=fused, stats=dp.comm.stats() if fused else (0, 0)), os.environ["OUT"])
    if use_dp:
        dist.barrier(); dist.destroy_process_group()
print("OK")
'''


def _worker(tmp_path, name, env_extra):
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    out = str(tmp_path / name)
    env = dict(os.environ, REPO_ROOT=ROOT, OUT=out, **env_extra)
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return torch.load(out), p.stderr


def test_deterministic_mode_bf16_runs_are_bit_identical_at_1024(tmp_path):
    """MB_DETERMINISTIC=1 at 16 heads (the r_w / r_r / r_s bias and seg_embed column sums of 16 heads, 1024-wide LayerNorm / bias slabs,
    the word scatter): two bf16 runs (dropout on, 4 single-call steps) in processes of their own end with the SAME bits, and so does
    the launch-by-launch call"""
    common = dict(JOB="det", MB_DETERMINISTIC="1")
    a, _ = _worker(tmp_path, "a.pt", dict(common, MODE="graph"))
    b, _ = _worker(tmp_path, "b.pt", dict(common, MODE="graph"))
    c, _ = _worker(tmp_path, "c.pt", dict(common, MODE="launches"))
    for other in (b, c):
        for k in ("p", "m", "v", "shadow"):
            assert torch.equal(a[k], other[k]), k
    assert float(a["g"].abs().max()) == 0.0


def test_single_call_dp_step_over_rccl_one_rank_at_24_x_1024(tmp_path):
    """mb_xlnet_train_step_dp at xlnet-large's depth -- 24 layers: pieces of 4 | 4 | 4 | 4 | 4 | 2 | 2 layers, nine segments -- over a
    one-rank RCCL communicator: every collective is an identity, so in deterministic mode fp32 parameters after three steps are
    bit-identical to the plain single-call step (the rule of test_dp_gpu.test_single_call_dp_step_over_rccl_one_rank)"""
    from conftest import free_port
    common = dict(JOB="dp", MB_DETERMINISTIC="1", MB_DP_FORCE="1", MB_DP_GRAD_DTYPE="fp32", RANK="0", WORLD_SIZE="1",
                  MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    a, _ = _worker(tmp_path, "plain.pt", dict(common, USE_DP="0", MASTER_PORT=str(free_port())))
    b, _ = _worker(tmp_path, "dp.pt", dict(common, USE_DP="1", MASTER_PORT=str(free_port())))
    assert b["fused"] and not a["fused"]
    print("24 x 1024, one-rank RCCL: %d collectives, %.1f MB; max |dparam| %.3e" % (b["stats"][0], b["stats"][1] * 1e-6,
                                                                                    float((a["p"] - b["p"]).abs().max())))
    assert b["stats"][0] >= 7
    assert torch.equal(a["p"], b["p"])


# ------------------------------------------------------------------------------------------------------------ 14. - 17. checkpoint, surfaces
def test_checkpoint_resumes_bit_equal_at_1024(tmp_path, monkeypatch):
    """2 x 1024: state_dict + optimizer state + dropout counter after 2 steps into fresh objects: step 3 is bit-equal to the
    uninterrupted run (deterministic mode, bf16, dropout on)"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    kw = dict(shapes=((5, 50),), p=0.1, p_mag=0.5)
    run = _steps(1024, 2, torch.bfloat16, True, nsteps=2, **kw)
    m, opt, sch = run["model"], run["opt"], run["sch"]
    path = str(tmp_path / "ckpt.pt")
    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}, "opt": opt.state_dict(), "sch": sch.state_dict(),
                "rng": m.get_rng_state()}, path)
    b3 = weights.synthetic_xlnet_batch(5, 50, 47, 74, seed=52)
    m.train_step(*tb(b3, DEV), optimizer=opt, graph=True)
    torch.cuda.synchronize()
    want = (m.flat_params.clone(), m._core._adam_m.clone(), m._core._adam_v.clone())
    del run, m, opt, sch
    fresh = _steps(1024, 2, torch.bfloat16, True, nsteps=0, **kw)
    m2, opt2, sch2 = fresh["model"], fresh["opt"], fresh["sch"]
    ck = torch.load(path)
    m2.load_state_dict(ck["model"]); opt2.load_state_dict(ck["opt"]); sch2.load_state_dict(ck["sch"]); m2.set_rng_state(ck["rng"])
    m2.train_step(*tb(b3, DEV), optimizer=opt2, graph=True)
    torch.cuda.synchronize()
    for x, y in zip(want, (m2.flat_params, m2._core._adam_m, m2._core._adam_v)):
        assert torch.equal(x, y)


def test_from_pretrained_reads_the_config_json_of_a_large_checkpoint(tmp_path):
    src = make(1024, 2, torch.float32)
    torch.save({k: v.cpu() for k, v in src.state_dict().items() if k.startswith("transformer.")}, tmp_path / "pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps(dict(size_config(1024, 2), model_type="xlnet", vocab_size=32000, untie_r=True,
                                                          architectures=["XLNetLMHeadModel"], ff_activation="gelu", attn_type="bi")))
    p = MAG_XLNetForSequenceClassification.from_pretrained(str(tmp_path), multimodal_config=MultimodalConfig(1.0, 0.0), visual_dim=47, acoustic_dim=74)
    assert (p.config.d_model, p.config.n_head, p.config.n_layer, p.config.d_inner) == (1024, 16, 2, 4096)
    for k, v in src.state_dict().items():
        if k.startswith("transformer.") and not k.startswith("transformer.MAG."):
            assert torch.equal(p.state_dict()[k], v), k
    b = weights.synthetic_xlnet_batch(3, 24, 47, 74, seed=2)
    assert bool(torch.isfinite(eval_logits(p.eval(), b)).all())


def test_driver_runs_xlnet_large():
    r = subprocess.run([sys.executable, "-m", "bert_multimodal_transformer_amd.multimodal_driver", "--model", "xlnet-large-cased",
                        "--synthetic", "192", "--n_epochs", "1"], cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import re
    losses = [float(x) for x in re.findall(r"train_loss[:=]\s*([-+0-9.eE]+|nan|inf)", r.stdout)]
    assert "nan" not in r.stdout.lower() and all(np.isfinite(losses)), r.stdout[-2000:]


def test_argument_checks():
    """a width the engine does not run raises the ValueError naming the four from Python, not an engine error code; so does an
    injection_index behind the last layer"""
    with pytest.raises(ValueError) as ei:
        MAG_XLNetForSequenceClassification(XLNetConfig(d_model=640, n_head=10, d_inner=2560, n_layer=2), MultimodalConfig(1.0, 0.5))
    assert "256, 512, 768, 1024" in str(ei.value)
    with pytest.raises(ValueError):
        MAG_XLNetForSequenceClassification(XLNetConfig(d_model=1024, n_head=12, d_inner=4096, n_layer=2), MultimodalConfig(1.0, 0.5))
    with pytest.raises(ValueError, match="injection_index"):
        MAG_XLNetForSequenceClassification(XLNetConfig(n_layer=2, **{k: v for k, v in size_config(1024).items() if k != "n_layer"}),
                                           MultimodalConfig(1.0, 0.5), injection_index=2)
    m = make(1024, 2).eval()                                        # mems of another width are refused by shape
    ids, vis, aco, mask, seg, _ = tb(weights.synthetic_xlnet_batch(2, 24, 47, 74, seed=3), DEV)
    with torch.no_grad(), pytest.raises(ValueError):
        m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, mems=[torch.zeros(16, 2, 768) for _ in range(2)])
