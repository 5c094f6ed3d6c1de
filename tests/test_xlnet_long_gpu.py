"""GPU: MAG-XLNet on sequences longer than 128 rows (the tiled relative-attention kernels, csrc/xlnet_attention_tiled.hip).

Op level: the tiled kernels against an fp64 torch restatement of the relative-attention formulas written here (bounds of
test_ops_gpu.close with the factors the MAG-BERT tiled test uses) and, at L <= 128, against the LDS-resident kernels through the same
library.  Model level: the live CPU oracle (oracle/mag_xlnet_ref.py), which has no length-specific code, and one fixture written by
the reference's own xlnet.py (tests/golden/g10_xlnet_long.npz, scripts/make_golden_long.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, MAG_XLNetForSequenceClassification, MultimodalConfig, XLNetConfig, _lib,
                                             get_linear_schedule_with_warmup, rng)
from oracle import mag_xlnet_ref as X
from oracle import optim_ref as O
from oracle import weights
from attn_op_helpers import NAMES, _XlOp, _errors, _xl_ref          # noqa: F401
from test_ops_gpu import close, rnd, stream
from test_xlnet_gpu import DEV, LOOSE_BF16, _grad_report, oracle, tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = [(_lib.DT_F32, torch.float32), (_lib.DT_BF16, torch.bfloat16)]


sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_long import long_batch          # noqa: E402  (ONE construction for the fixture's generator and the tests)


def make(layers=12, cdt=torch.float32, p_mag=0.5, p=0.1, max_seq_length=512, mem_len=None):
    cfg = XLNetConfig(n_layer=layers, num_labels=1, dropout=p, summary_last_dropout=p, mem_len=mem_len)
    m = MAG_XLNetForSequenceClassification(cfg, MultimodalConfig(1.0, p_mag), visual_dim=47, acoustic_dim=74, compute_dtype=cdt,
                                           max_seq_length=max_seq_length)
    m.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(q.shape), "test")) for n, q in m.named_parameters()})
    return m


def eval_logits(m, b, **kw):
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    with torch.no_grad():
        return m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, **kw)[0].float().cpu()


def oracle_logits(o, b, **kw):
    i2, v2, a2, m2, s2, _ = tb(b)
    with torch.no_grad():
        return o(i2, v2, a2, m2, s2, **kw)[0]


# ------------------------------------------------------------------------------------------------------------ op level
# (_xl_ref, _XlOp, _errors, NAMES: attn_op_helpers.py, shared with test_attention_resident_gpu.py)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [64, 128, 129, 200, 256, 384, 512])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_tiled_relative_attention_vs_fp64(dt, tdt, L, p):
    """forward vec, dq | dk | dv, dkr and the four parameter gradients against fp64; B = 2 with row 0 at full length and row 1
    left-padded down to 5 real keys, a head_scale with one zero, segment ids of both kinds.  Bound: test_ops_gpu.close() times 2
    (forward) / 3 (backward), the factors of the MAG-BERT tiled test.  Reruns are bit-identical in everything that has one writer."""
    case = _XlOp(dt, tdt, 2, L, 12, 11, p)
    ref_vec, ref_grads = case.reference()
    got = case.run(tiled=True)
    for k, (e, s) in _errors(case, got, ref_vec, ref_grads).items():
        print("tiled xlnet attention %s L=%d p=%g %s: max|err| %.3e (max|ref| %.3e)" % (tdt, L, p, k, e, s))
    vec, dqkv, dkr, pg = got
    close(vec.float(), ref_vec.float(), dt, "tiled fwd", 2.0)
    close(dqkv.float(), ref_grads[0].float(), dt, "tiled dq|dk|dv", 3.0)
    close(dkr.float(), ref_grads[1].float(), dt, "tiled dkr", 3.0)
    for name, g, r in zip(NAMES[2:], pg, ref_grads[2:]):
        close(g, r.float().view(g.shape), dt, "tiled " + name, 3.0)
    a, b = case.run(tiled=True), case.run(tiled=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    if L <= 128:            # the LDS-resident kernels on the same inputs, through the same library
        res = case.run(tiled=False)
        close(vec.float(), res[0].float().cpu(), dt, "tiled vs resident fwd", 2.0)
        close(dqkv.float(), res[1].float().cpu(), dt, "tiled vs resident dq|dk|dv", 3.0)
        close(dkr.float(), res[2].float().cpu(), dt, "tiled vs resident dkr", 3.0)
        for name, g, r in zip(NAMES[2:], pg, res[3]):
            close(g, r.cpu(), dt, "tiled vs resident " + name, 3.0)


@pytest.mark.parametrize("dt,tdt", DTS)
def test_tiled_relative_attention_perm_mask_vs_fp64(dt, tdt):
    """a random perm (30 %) next to the padding at L = 200, dropout on: the backward recomputes the scores, so it applies perm itself"""
    case = _XlOp(dt, tdt, 2, 200, 12, 23, 0.1, perm=True)
    ref_vec, ref_grads = case.reference()
    vec, dqkv, dkr, pg = case.run(tiled=True)
    close(vec.float(), ref_vec.float(), dt, "perm fwd", 2.0)
    close(dqkv.float(), ref_grads[0].float(), dt, "perm dq|dk|dv", 3.0)
    close(dkr.float(), ref_grads[1].float(), dt, "perm dkr", 3.0)
    for name, g, r in zip(NAMES[2:], pg, ref_grads[2:]):
        close(g, r.float().view(g.shape), dt, "perm " + name, 3.0)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [100, 300])
def test_tiled_query_stream_mask_with_a_fully_masked_row(dt, tdt, L):
    """gstream = 1 (no self exemption): a row whose every key is masked yields the uniform distribution over the L keys -- columns
    beyond L in the last tile must weigh nothing.  Forward only (the query stream has no backward).  At L <= 128 the LDS-resident
    kernels run the same inputs and every row of the two outputs is compared, the fully masked rows included."""
    case = _XlOp(dt, tdt, 2, L, 12, 31, 0.0, gstream=1)
    ref_vec, _ = case.reference(backward=False)
    vec = case.run(tiled=True, backward=False)[0]
    close(vec.float(), ref_vec.float(), dt, "gstream fwd", 2.0)
    v = case.qkv.double().view(2, L, 3, 12, 64)[0, :, 2].mean(0) * case.hs.double()[:, None]              # uniform over all L keys
    close(vec.float().view(2, L, 12, 64)[0, L // 2], v.float(), dt, "fully masked row", 2.0)
    if L <= 128:
        # the LDS-resident kernels on the same inputs: every row, the two fully masked ones included (they pad with -inf as the tiled
        # kernels do; with -1e30, XLNet's own mask value, such a row spread its weight over LP columns and returned L / LP of this)
        res = case.run(tiled=False, backward=False)[0].float().cpu().view(2, L, 12 * 64)
        got = vec.float().cpu().view(2, L, 12 * 64)
        full = torch.zeros(2, L, dtype=torch.bool)
        full[0, L // 2] = True
        full[1, L - 2] = True
        print("gstream L=%d %s: resident vs fp64 on the fully masked rows %.3e (max|ref| %.3e), tiled %.3e"
              % (L, tdt, float((res[full].double() - ref_vec.view(2, L, -1)[full]).abs().max()), float(ref_vec.view(2, L, -1)[full].abs().max()),
                 float((got[full].double() - ref_vec.view(2, L, -1)[full]).abs().max())))
        close(got, res, dt, "gstream tiled vs resident", 2.0)


# ------------------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("cdt,B,L,layers,tol", [(torch.float32, 2, 256, 2, 1e-3), (torch.float32, 3, 300, 2, 1e-3),
                                                (torch.float32, 2, 512, 12, 1e-3), (torch.bfloat16, 2, 512, 12, 5e-2)])
def test_long_eval_logits_vs_oracle(cdt, B, L, layers, tol):
    m, o = make(layers, cdt).eval(), oracle(layers).eval()
    b = long_batch(B, L, seed=200 + L)
    err = float((eval_logits(m, b) - oracle_logits(o, b)).abs().max())
    print("xlnet eval B=%d L=%d layers=%d %s: logits %.2e" % (B, L, layers, cdt, err))
    assert err <= tol


@pytest.mark.parametrize("B,L,seed", [(2, 256, 51), (2, 512, 53)])
def test_long_eval_logits_match_reference_golden_fp32(golden, B, L, seed):
    """what the reference's own xlnet.py returned (scripts/make_golden_long.py)"""
    m = make(12).eval()
    ref = golden["g10_xlnet_long"]["logits/B%d_L%d_seed%d" % (B, L, seed)]
    err = float(np.abs(eval_logits(m, long_batch(B, L, seed)).numpy() - ref).max())
    print("xlnet eval vs reference golden B=%d L=%d: %.2e" % (B, L, err))
    assert err <= 1e-3


def _replay_oracle(layers, B, L, core):
    """the oracle in train mode with every dropout module replaying the device masks of the engine's last pass (host-regenerated
    from its seed and step), as test_xlnet_gpu.oracle_replay_grads builds it -- returned as a module, so that its attention
    probabilities can be read after the pass"""
    from test_xlnet_gpu import _SeqReplay as S
    o = oracle(layers).train()
    nh, H, DI = 12, 768, 3072
    mult = lambda site, p, n: torch.from_numpy(rng.keep_mult(n, rng.make_key(core.seed, core.step, site, p)))
    blx = lambda site, p, Xd: mult(site, p, B * L * Xd).view(B, L, Xd).permute(1, 0, 2)
    o.transformer.dropout = S([blx(rng.XS_EMB, 0.1, H), mult(rng.XS_POS, 0.1, 2 * L * B * H).view(2 * L, B, H), blx(rng.XS_FINAL, 0.1, H)])
    o.transformer.MAG.dropout = S([blx(rng.XS_MAG, 0.5, H)])
    o.sequence_summary.last_dropout = S([mult(rng.XS_HEAD, 0.1, B * H).view(B, H)])
    for l, lyr in enumerate(o.transformer.layer):
        s0 = rng.XS_LAYER0 + 8 * l
        lyr.rel_attn.dropout = S([mult(s0 + 0, 0.1, B * nh * L * L).view(B, nh, L, L), blx(s0 + 1, 0.1, H)])
        lyr.ff.dropout = S([blx(s0 + 2, 0.1, DI), blx(s0 + 3, 0.1, H)])
    return o


@pytest.mark.parametrize("cdt,tol_logit,tol_grad,tol_prob", [(torch.float32, 1e-3, 5e-3, 1e-5), (torch.bfloat16, 5e-2, 1e-1, 2e-2)])
def test_long_train_mode_dropout_mask_replay(cdt, tol_logit, tol_grad, tol_prob):
    """2 layers, B = 2, L = 256, dropout ON at every site with the device masks replayed inside the oracle (bounds of
    test_xlnet_gpu.test_train_mode_dropout_mask_replay): logits, the attention probabilities after dropout -- above 128 rows a
    recomputation, mb_xlnet_attention_probs_into --, the hidden states' shape, every gradient."""
    layers, B, L = 2, 2, 256
    torch.manual_seed(99)          # pinned: see test_train_mode_dropout_mask_replay
    m = make(layers, cdt).train()
    b = long_batch(B, L, seed=141)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    out = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None, output_attentions=True, output_hidden_states=True)
    logits, hid, att = out[0], out[1], out[2]
    F.mse_loss(logits.view(-1), lab.view(-1)).backward()
    o = _replay_oracle(layers, B, L, m._core)
    i2, v2, a2, m2, s2, l2 = tb(b)
    lo = o(i2, v2, a2, m2, s2)[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu() - lo.detach()).abs().max())
    perr = max(float((att[l].cpu() - lyr.rel_attn.last_probs.detach()).abs().max()) for l, lyr in enumerate(o.transformer.layer))
    print("xlnet long train-mode %s: logits %.2e, probabilities after dropout %.2e" % (cdt, err, perr))
    assert err <= tol_logit and perr <= tol_prob
    assert len(att) == layers and tuple(att[0].shape) == (B, 12, L, L)
    assert len(hid) == layers + 1 and tuple(hid[0].shape) == (B, L, 768)
    _grad_report(m, o, tol_grad, frobenius=(cdt == torch.bfloat16))


def test_long_fused_step_bf16_full_model_vs_oracle():
    """12 layers, B = 8, L = 512, bf16, dropout on, through the fused training step (what train_epoch calls): loss 5e-3 relative,
    gradients 3e-2 relative Frobenius, MAG's four gated tensors 1e-1 (the bounds of test_train_mode_dropout_mask_replay's 12-layer legs)"""
    layers, B, L = 12, 8, 512
    torch.manual_seed(99)
    m = make(layers, torch.bfloat16).train()
    b = long_batch(B, L, seed=143)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    loss = m.training_step(ids, vis, aco, mask, seg, lab)
    o = _replay_oracle(layers, B, L, m._core)
    i2, v2, a2, m2, s2, l2 = tb(b)
    loss_o = F.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1))
    loss_o.backward()
    torch.cuda.synchronize()
    print("xlnet long fused step bf16: loss %.6f vs oracle %.6f" % (float(loss), float(loss_o)))
    assert abs(float(loss) - float(loss_o)) <= 5e-3 * max(1.0, abs(float(loss_o)))
    _grad_report(m, o, 3e-2, frobenius=True, loose=LOOSE_BF16, tol_loose=1e-1, show=6)


@pytest.mark.parametrize("L,ml", [(200, 200), (256, 256)])
def test_long_mems_eval_vs_oracle_fp32(L, ml):
    """two segments, klen = 400 and 512: logits of the segment that consumes memories and the memories it caches, vs the oracle"""
    layers, B = 2, 2
    m = make(layers, mem_len=ml).eval()
    o = oracle(layers).eval()
    b1, b2 = long_batch(B, L, seed=150), long_batch(B, L, seed=151)
    i1, v1, a1, m1, s1, _ = tb(b1, DEV)
    i2, v2, a2, m2, s2, _ = tb(b2, DEV)
    with torch.no_grad():
        r1 = m(i1, v1, a1, token_type_ids=s1, attention_mask=m1, use_cache=True)
        r2 = m(i2, v2, a2, token_type_ids=s2, attention_mask=m2, use_cache=True, mems=list(r1[1]))
        c1, c2 = tb(b1), tb(b2)
        o1 = o(c1[0], c1[1], c1[2], c1[3], c1[4], mem_len=ml)[0]
        mems1 = [t.clone() for t in o.transformer.new_mems]
        o2 = o(c2[0], c2[1], c2[2], c2[3], c2[4], mems=mems1, mem_len=ml)[0]
        mems2 = [t.clone() for t in o.transformer.new_mems]
        plain = o(c2[0], c2[1], c2[2], c2[3], c2[4])[0]
    e1, e2 = float((r1[0].cpu() - o1).abs().max()), float((r2[0].cpu() - o2).abs().max())
    em = max(float((a.cpu() - b_).abs().max()) for a, b_ in zip(r2[1], mems2))
    print("xlnet long mems klen=%d: logits %.2e / %.2e, new_mems %.2e (the memory moves the logits by %.2e)"
          % (L + ml, e1, e2, em, float((o2 - plain).abs().max())))
    assert e1 <= 1e-3 and e2 <= 1e-3 and em <= 1e-3
    assert tuple(r2[1][0].shape) == (ml, B, 768)


def test_long_mems_training_gradients_and_limit_fp32():
    """training with memories at klen = 400 (5e-3 as test_mems_training_gradients_vs_oracle); klen = 513 raises NotImplementedError"""
    layers, B, L, ml = 2, 2, 200, 200
    m = make(layers, p_mag=0.0, p=0.0).train()
    o = X.set_dropout(oracle(layers, p_mag=0.0), 0.0, 0.0).train()
    b = long_batch(B, L, seed=152)
    g = torch.Generator().manual_seed(5)
    mems = [torch.randn(ml, B, 768, generator=g) * 0.5 for _ in range(layers)]
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, mems=[t.to(DEV) for t in mems], labels=None)[0]
    F.mse_loss(logits.view(-1), lab.view(-1)).backward()
    i2, v2, a2, m2, s2, l2 = tb(b)
    lo = o(i2, v2, a2, m2, s2, mems=mems)[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu() - lo.detach()).abs().max())
    print("xlnet long mems training klen=400: logits %.2e" % err)
    assert err <= 1e-3
    _grad_report(m, o, 5e-3, show=3)
    big = [torch.zeros(313, B, 768) for _ in range(layers)]
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, mems=big)


@pytest.mark.parametrize("B,L,M", [(2, 256, 9), (2, 512, 5)])
def test_long_query_stream_vs_oracle_fp32(B, L, M):
    """target_mapping with the "nobody sees a target" perm_mask of make_golden.gen_xlnet: output_g and logits vs the oracle"""
    layers = 2
    m, o = make(layers).eval(), oracle(layers).eval()
    b = long_batch(B, L, seed=160 + M, short=2 * M)          # (the short row needs M real positions to draw its targets from)
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    rs = np.random.RandomState(L)
    tm, pm = np.zeros((B, M, L), np.float32), np.zeros((B, L, L), np.float32)
    for r in range(B):
        real = np.flatnonzero(b["input_mask"][r] > 0)
        tgt = np.sort(rs.choice(real, size=M, replace=False))
        tm[r, np.arange(M), tgt] = 1.0
        pm[r][:, tgt] = 1.0
    tm_t, pm_t = torch.from_numpy(tm), torch.from_numpy(pm)
    with torch.no_grad():
        out_g = m.transformer(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t.to(DEV), target_mapping=tm_t.to(DEV))[0].cpu()
        logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t.to(DEV), target_mapping=tm_t.to(DEV))[0].cpu()
        i2, v2, a2, m2, s2, _ = tb(b)
        ref_g = o.transformer(i2, v2, a2, m2, s2, perm_mask=pm_t, target_mapping=tm_t)
        ref_l = o(i2, v2, a2, m2, s2, perm_mask=pm_t, target_mapping=tm_t)[0]
    ref_g = ref_g[0] if isinstance(ref_g, (tuple, list)) else ref_g
    e_g, e_l = float((out_g - ref_g).abs().max()), float((logits - ref_l).abs().max())
    print("xlnet long query stream B=%d L=%d M=%d: output_g %.2e, logits %.2e" % (B, L, M, e_g, e_l))
    assert tuple(out_g.shape) == (B, M, 768) and e_g <= 1e-3 and e_l <= 1e-3


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_long_perm_mask_and_head_mask_gradients_vs_oracle(cdt):
    """L = 256, train mode with every dropout p = 0: a random perm_mask next to the padding (bounds of
    test_perm_mask_gradients_vs_oracle), the same with input_mask instead of attention_mask, then a head_mask with zeros"""
    layers, B, L, nh = 2, 2, 256, 12
    fp32 = cdt == torch.float32
    m = make(layers, cdt, p_mag=0.0, p=0.0).train()
    o = X.set_dropout(oracle(layers, p_mag=0.0), 0.0, 0.0).train()
    b = long_batch(B, L, seed=158)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    i2, v2, a2, m2, s2, l2 = tb(b)
    perm = torch.from_numpy((np.random.RandomState(3).rand(B, L, L) < 0.4).astype(np.float32))
    logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=perm.to(DEV))[0]
    F.mse_loss(logits.view(-1), lab.view(-1)).backward()
    lo = o(i2, v2, a2, m2, s2, perm_mask=perm)[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu() - lo.detach()).abs().max())
    print("xlnet long perm_mask (%s): logits %.2e" % (cdt, err))
    assert err <= (1e-3 if fp32 else 5e-2)
    _grad_report(m, o, 5e-3 if fp32 else 1e-1, frobenius=not fp32)
    # input_mask, the reference's inverse spelling of attention_mask (xlnet.py:258-264), alone and next to the perm_mask
    m.zero_grad(); o.zero_grad()
    im_d, im = 1.0 - mask.float(), 1.0 - m2.float()
    logits = m(ids, vis, aco, token_type_ids=seg, input_mask=im_d, perm_mask=perm.to(DEV))[0]
    F.mse_loss(logits.view(-1), lab.view(-1)).backward()
    lo = o(i2, v2, a2, None, s2, perm_mask=perm, input_mask=im)[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu() - lo.detach()).abs().max())
    with torch.no_grad():
        e2 = float((m(ids, vis, aco, token_type_ids=seg, input_mask=im_d)[0].cpu() - o(i2, v2, a2, None, s2, input_mask=im)[0]).abs().max())
    print("xlnet long input_mask (%s): logits with perm_mask %.2e, alone %.2e" % (cdt, err, e2))
    assert max(err, e2) <= (1e-3 if fp32 else 5e-2)
    _grad_report(m, o, 5e-3 if fp32 else 1e-1, frobenius=not fp32)
    m.zero_grad(); o.zero_grad()
    hm = torch.ones(layers, nh)
    hm[0, 2] = 0.0; hm[0, 9] = 0.5; hm[1, 0] = 0.0; hm[1, 5] = 2.0
    logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, head_mask=hm.to(DEV))[0]
    F.mse_loss(logits.view(-1), lab.view(-1)).backward()
    lo = o(i2, v2, a2, m2, s2, head_mask=hm)[0]
    F.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu() - lo.detach()).abs().max())
    print("xlnet long head_mask (%s): logits %.2e" % (cdt, err))
    assert err <= (1e-3 if fp32 else 5e-2)
    _grad_report(m, o, 5e-3 if fp32 else 1e-1, frobenius=not fp32)


def test_long_three_optimizer_steps_track_the_oracle_fp32():
    """three AdamW steps at L = 200 through the single-call step, mb_xlnet_train_step, as ONE replayed graph per step (graph=True
    raises if the single call is unavailable; the engine's graph counters are read back): bounds of
    test_three_optimizer_steps_track_the_oracle_fp32 -- parameters 2e-4 after the steps, eval logits 5e-3 afterwards"""
    layers = 2
    m = make(layers, p_mag=0.0, p=0.0).train()
    o = X.set_dropout(oracle(layers, p_mag=0.0), 0.0, 0.0).train()
    from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
    opt = AdamW(optimizer_grouped_parameters(m), lr=1e-3)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    oo = O.AdamW(O.grouped_parameters(o), lr=1e-3)
    so = O.get_linear_schedule_with_warmup(oo, num_warmup_steps=1.0, num_training_steps=10)
    with m.stream_scope():
        for s in range(3):
            b = long_batch(2, 200, seed=170 + s)
            ids, vis, aco, mask, seg, lab = tb(b, DEV)
            m.train_step(ids, vis, aco, mask, seg, lab, optimizer=opt, graph=True)
            sch.step()
            i2, v2, a2, m2, s2, l2 = tb(b)
            oo.zero_grad()
            F.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1)).backward()
            oo.step(); so.step()
    torch.cuda.synchronize()
    cap, rep = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.lib().mb_xlnet_graph_stats(m._core.handle, C.byref(cap), C.byref(rep)))
    print("xlnet long single-call steps: graph captures %d, replays %d" % (cap.value, rep.value))
    assert cap.value >= 1 and rep.value >= 3
    om = dict(o.named_parameters())
    worst = max(float((p.detach().cpu() - om[n].detach()).abs().max()) for n, p in m.named_parameters())
    print("xlnet long: max |param - oracle param| after 3 steps:", worst)
    assert worst <= 2e-4
    m.eval(); o.eval()
    b = long_batch(2, 200, seed=175)
    e = float((eval_logits(m, b) - oracle_logits(o, b)).abs().max())
    print("xlnet long: eval logits after the steps %.2e" % e)
    assert e <= 5e-3


_DET_WORKER = r"""
import os, sys, torch
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from test_xlnet_long_gpu import make, long_batch, tb, DEV
from bert_multimodal_transformer_amd import AdamW, get_linear_schedule_with_warmup
from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
torch.manual_seed(7)
m = make(2, torch.bfloat16).train()
opt = AdamW(optimizer_grouped_parameters(m), lr=1e-3)
sch = get_linear_schedule_with_warmup(opt, 0, 100)
with m.stream_scope():
    for s in range(3):
        ids, vis, aco, mask, seg, lab = tb(long_batch(2, 256, seed=180 + s), DEV)
        m.train_step(ids, vis, aco, mask, seg, lab, optimizer=opt, graph=True if sys.argv[3] == "graph" else "launches")
        sch.step()
torch.cuda.synchronize()
core = m._core
torch.save({"p": core.params.cpu(), "m": core._adam_m.cpu(), "v": core._adam_v.cpu(), "sh": core.shadow.cpu()}, sys.argv[2])
"""


def test_long_deterministic_mode_graph_and_eager_are_bit_identical_bf16(tmp_path):
    """MB_DETERMINISTIC=1, bf16, L = 256, three optimizer steps through the single-call step: two runs, the launch-by-launch form
    (graph="launches"), a run with an MB_ADAMW_RIDE_* override (the tiled launches take no riders whatever it says) and a run without
    riders (MB_ADAMW_RIDE=0) all end in the same bits -- parameters, both moments, the bf16 shadow"""
    outs = []
    for k, (mode, extra) in enumerate((("graph", {}), ("graph", {}), ("launches", {}), ("graph", {"MB_ADAMW_RIDE_ATTN_BLOCKS": "64"}),
                                       ("graph", {"MB_ADAMW_RIDE": "0"}))):
        env = dict(os.environ, MB_DETERMINISTIC="1", **extra)
        f = str(tmp_path / ("run%d.pt" % k))
        r = subprocess.run([sys.executable, "-c", _DET_WORKER, ROOT, f, mode], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(torch.load(f))
    for k in range(1, len(outs)):
        for name in ("p", "m", "v", "sh"):
            assert torch.equal(outs[0][name], outs[k][name]), (k, name)


# ------------------------------------------------------------------------------------------------------------ limits
def test_limits_and_untouched_ground():
    """a max_seq_length = 512 model gives the default model's bits at L = 50 (bf16 eval); a default model still refuses L = 130; 513 is
    a ValueError; a batch longer than the model's limit raises MagbertError naming max_seq_length"""
    b = weights.synthetic_xlnet_batch(4, 50, 47, 74, seed=31)
    big = make(2, torch.bfloat16, max_seq_length=512).eval()
    eval_logits(big, long_batch(2, 200, seed=1))           # the engine is built for long sequences before the short pass
    small = make(2, torch.bfloat16, max_seq_length=None).eval()
    assert torch.equal(eval_logits(big, b), eval_logits(small, b))
    with pytest.raises(_lib.MagbertError, match="max_seq_length"):
        eval_logits(small, long_batch(2, 130, seed=1))
    with pytest.raises(ValueError):
        make(2, max_seq_length=513)
    mid = make(2, max_seq_length=256).eval()
    with pytest.raises(_lib.MagbertError, match="max_seq_length"):
        eval_logits(mid, long_batch(2, 300, seed=1))
    eval_logits(mid, long_batch(2, 256, seed=1))


def test_from_pretrained_forwards_max_seq_length(tmp_path):
    m = make(2)          # (MAG sits in front of layer 1: two layers at least)
    torch.save({k: v.cpu() for k, v in m.state_dict().items() if k.startswith("transformer.")}, tmp_path / "pytorch_model.bin")
    m2 = MAG_XLNetForSequenceClassification.from_pretrained(str(tmp_path), config=XLNetConfig(n_layer=2, num_labels=1),
                                                            multimodal_config=MultimodalConfig(1.0, 0.5), visual_dim=47, acoustic_dim=74,
                                                            max_seq_length=300)
    assert m2._core.max_seq_length == 300
    assert bool(torch.isfinite(eval_logits(m2.eval(), long_batch(2, 300, seed=2))).all())


def test_dev_batch_eval_bf16_is_finite_and_matches_the_oracle_rows():
    """the driver's dev batch at the longest length: B = 128, L = 512, bf16, 12 layers"""
    B, L = 128, 512
    m, o = make(12, torch.bfloat16).eval(), oracle(12).eval()
    b = long_batch(B, L, seed=190)
    got = eval_logits(m, b)
    assert bool(torch.isfinite(got).all())
    b4 = {k: v[:4] for k, v in b.items()}
    err = float((got[:4] - oracle_logits(o, b4)).abs().max())
    print("xlnet dev batch B=128 L=512 bf16: first four rows vs the oracle %.2e" % err)
    assert err <= 5e-2


def test_driver_runs_at_256():
    r = subprocess.run([sys.executable, "-m", "bert_multimodal_transformer_amd.multimodal_driver", "--model", "xlnet-base-cased", "--synthetic", "96",
                        "--max_seq_length", "256", "--n_epochs", "1", "--train_batch_size", "16"], cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
