"""GPU: MAG-BERT at the hidden sizes next to bert-base -- 256 (4 heads), 512 (8 heads) and 1024 (16 heads, bert-large-uncased).

References: tests/golden/g11_bert_sizes.npz (the reference's own logits at full depth: scripts/make_golden_sizes.py) and the CPU oracle
run live on the same inputs.  Bounds are the project's: fp32 logits 1e-3, fp32 gradients 5e-3 of the tensor's max, bf16 at 2 layers
logits 1e-2 / gradients 3e-2 relative Frobenius (MAG's gated tensors 1e-1) as in test_model_gpu; at full depth the bf16 logit bound is
2e-2 -- the bound of the benchmarked 12 x 768 step -- scaled by the oracle's own bf16-autocast error at the new size over its autocast
error at 12 x 768 on the same batch (never below 2e-2), both computed live."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import AdamW, BertConfig, MAG_BertForSequenceClassification, MultimodalConfig, _lib
from bert_multimodal_transformer_amd import get_linear_schedule_with_warmup
from oracle import mag_bert_ref as R, optim_ref as O, weights
from test_model_gpu import DEV, LOOSE_BF16, _grad_report, tb
from test_ops_gpu import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_sizes import CASES, SAMPLE, SIZES, key, size_config      # noqa: E402

NEW = [s[0] for s in SIZES]          # 1024, 512, 256


def make(H, layers=None, cdt=torch.float32, V=47, p_mag=0.0, hidden_p=0.0, attn_p=0.0, num_labels=1, max_seq_length=None):
    cfg = BertConfig(hidden_dropout_prob=hidden_p, attention_probs_dropout_prob=attn_p, **size_config(H, layers, num_labels))
    m = MAG_BertForSequenceClassification(cfg, MultimodalConfig(1.0, p_mag), visual_dim=V, acoustic_dim=74, compute_dtype=cdt,
                                          max_seq_length=max_seq_length)
    m.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(p.shape), "test")) for n, p in m.named_parameters()})
    return m


def oracle(H, layers=None, V=47, p_mag=0.0, num_labels=1):
    kw = size_config(H, layers, num_labels) if H != 768 else dict(num_hidden_layers=12 if layers is None else layers, num_labels=num_labels)
    o = R.MAG_BertForSequenceClassification(R.BertConfigLite(**kw), R.MultimodalConfig(1.0, p_mag), V, 74)
    return R.set_dropout(R.load_deterministic(o, "test"), 0.0, 0.0, 0.0)


def eval_logits(m, b):
    ids, vis, aco, mask, seg, _ = tb(b, DEV)
    with torch.no_grad():
        return m(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0].float().cpu()


def oracle_logits(o, b, **kw):
    i2, v2, a2, m2, s2, _ = tb(b)
    with torch.no_grad():
        return o(i2, v2, a2, m2, s2, **kw)[0]


# ------------------------------------------------------------------------------------------------------------ head kernels
@pytest.mark.parametrize("cdt,dt", [(torch.float32, _lib.DT_F32), (torch.bfloat16, _lib.DT_BF16)])
@pytest.mark.parametrize("nl", [1, 3])
@pytest.mark.parametrize("H", NEW)
def test_head_kernels_vs_fp64(H, nl, cdt, dt):
    """head_fwd / head_bwd at CH = H / 256 through a one-layer engine: logits, loss, and the gradients the head launch itself produces
    (classifier weight / bias, pooler bias; the pooler weight through the GEMM behind it) against fp64 torch on the engine's own last
    hidden state -- by the fused loss inside the kernel (labels) and by a dlogits handed in (autograd)."""
    B, L = 6, 8                                    # (6: the second block of four waves has two idle ones)
    m = make(H, 1, cdt, num_labels=nl).train()     # every dropout p = 0
    b = weights.synthetic_bert_batch(B, L, 47, 74, seed=7)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    y = lab if nl == 1 else torch.tensor([0, 2, 1, 1, 0, 2], device=DEV)
    loss = m.training_step(ids, vis, aco, mask, seg, y)
    x0 = m._core.hidden_states(B, L)[-1][:, 0].double().cpu()
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    Wp, bp = sd["bert.pooler.dense.weight"].requires_grad_(True), sd["bert.pooler.dense.bias"].requires_grad_(True)
    Wc, bc = sd["classifier.weight"].requires_grad_(True), sd["classifier.bias"].requires_grad_(True)
    if cdt == torch.bfloat16:                      # the pooler GEMM multiplies the bf16 shadow of its weight
        Wp = Wp.detach().to(torch.bfloat16).double().requires_grad_(True)
    ref_logits = torch.tanh(x0 @ Wp.T + bp) @ Wc.T + bc
    ref_loss = (torch.nn.functional.mse_loss(ref_logits.view(-1), y.double().cpu().view(-1)) if nl == 1
                else torch.nn.functional.cross_entropy(ref_logits, y.cpu()))
    ref_loss.backward()
    got = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    assert abs(float(loss) - float(ref_loss)) <= 2e-5 * max(1.0, abs(float(ref_loss))) * (1 if cdt == torch.float32 else 600)
    pairs = (("classifier.weight", Wc), ("classifier.bias", bc), ("bert.pooler.dense.bias", bp), ("bert.pooler.dense.weight", Wp))
    for n, r in pairs:
        close(got[n], r.grad, dt, "%s (fused loss)" % n, 4.0)
    # the same through autograd: forward -> logits, a dlogits from torch's loss -> head_bwd's dlogits branch
    m.zero_grad()
    out = m(ids, vis, aco, attention_mask=mask, token_type_ids=seg, labels=y)
    close(out[1].float(), ref_logits.detach(), dt, "logits", 4.0)
    out[0].backward()
    for n, r in pairs:
        close(dict(m.named_parameters())[n].grad, r.grad, dt, "%s (dlogits)" % n, 4.0)


# ------------------------------------------------------------------------------------------------------------ fp32 parity
@pytest.mark.parametrize("B,L,V,seed", CASES)
@pytest.mark.parametrize("H", NEW)
def test_fp32_logits_vs_reference_fixture_and_oracle(golden, H, B, L, V, seed):
    """full depth (24 x 1024, 8 x 512, 4 x 256), eval: the project's contract, |logit error| <= 1e-3"""
    g = golden["g11_bert_sizes"]
    m = make(H, None, torch.float32, V, p_mag=0.5).eval()
    b = weights.synthetic_bert_batch(B, L, V, 74, seed=seed)
    got = eval_logits(m, b)
    seq = m._core.sequence_output(B, L).float().cpu().numpy()
    err = float(np.abs(got.numpy() - g[key("logits", H, B, L, V, seed)]).max())
    err_seq = float(np.abs(weights.strided_sample(seq, SAMPLE) - g[key("seq", H, B, L, V, seed)]).max())
    live = float((got - oracle_logits(oracle(H, None, V).eval(), b)).abs().max())
    print("fp32 H=%d B=%d L=%d V=%d: logits max|err| vs fixture %.3e, vs live oracle %.3e; sequence_output sample %.3e" % (H, B, L, V, err, live, err_seq))
    assert err <= 1e-3 and live <= 1e-3 and err_seq <= 1e-3


@pytest.mark.parametrize("H,layers", [(256, 2), (512, 2), (1024, 2), (1024, None)])
def test_fp32_gradients_vs_oracle(H, layers):
    """train mode, every dropout p = 0: loss and ALL parameter gradients, 2 layers at each new size and bert-large at full depth"""
    m = make(H, layers, torch.float32).train()
    o = oracle(H, layers).train()
    b = weights.synthetic_bert_batch(4, 50, 47, 74, seed=21)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None)[0]
    loss = torch.nn.MSELoss()(logits.view(-1), lab.view(-1))
    loss.backward()
    i2, v2, a2, m2, s2, l2 = tb(b)
    lo = torch.nn.functional.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1))
    lo.backward()
    torch.cuda.synchronize()
    print("fp32 H=%d layers=%s: loss %.6f oracle %.6f" % (H, layers, float(loss), float(lo)))
    assert abs(float(loss) - float(lo)) < 1e-4
    _grad_report(m, o, 5e-3, show=3)
    # the fused step gives the same gradients (its loss lives inside the head kernel)
    g_ref = m.flat_grads.clone()
    m.zero_grad()
    l2_ = m.training_step(ids, vis, aco, mask, seg, lab)
    assert abs(float(l2_) - float(loss)) < 1e-5
    assert float((m.flat_grads - g_ref).abs().max()) <= 1e-5 * float(g_ref.abs().max()) + 1e-9


def test_optional_arguments_and_long_sequences_at_1024():
    """output_hidden_states, head_mask and L = 200 (max_seq_length = 256: the tiled attention path) at H = 1024, 16 heads"""
    H, layers, nh = 1024, 2, 16
    m = make(H, layers, torch.float32, max_seq_length=256).eval()
    o = oracle(H, layers).eval()
    for (B, L) in ((3, 40), (2, 200)):
        b = weights.synthetic_bert_batch(B, L, 47, 74, seed=83)
        b["input_mask"][0, :] = 1                     # row 0 at full length: at L = 200 the keys beyond 128 are live
        b["input_ids"][0, 1:L - 1] = 2000 + (np.arange(L - 2) * 7919) % 20000
        b["input_ids"][0, L - 1] = 102
        ids, vis, aco, mask, seg, _ = tb(b, DEV)
        i2, v2, a2, m2, s2, _ = tb(b)
        ref_h = []
        hooks = [o.bert.encoder.register_forward_pre_hook(lambda mod, args: ref_h.append(args[0].detach()))]
        for lyr in o.bert.encoder.layer:
            hooks.append(lyr.register_forward_hook(lambda mod, args, out: ref_h.append(out.detach())))
        with torch.no_grad():
            got = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, output_hidden_states=True, output_attentions=True)
            ref = o(i2, v2, a2, m2, s2)[0]
        for h in hooks:
            h.remove()
        logits, hs, att = got
        assert float((logits.cpu() - ref).abs().max()) <= 1e-3
        assert len(hs) == layers + 1 and tuple(hs[0].shape) == (B, L, H)
        for h, r in zip(hs, ref_h):
            assert float((h.cpu() - r).abs().max()) <= 1e-3
        assert len(att) == layers and tuple(att[0].shape) == (B, nh, L, L)
        for a, lyr in zip(att, o.bert.encoder.layer):
            assert float((a.cpu() - lyr.attention.self.last_probs).abs().max()) <= 1e-4
        hm = torch.ones(layers, nh)
        hm[0, 2] = 0.0
        hm[1, 15] = 0.5                               # the last of the 16 heads
        with torch.no_grad():
            g = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, head_mask=hm.to(DEV))[0].float().cpu()
        r = oracle_logits(o, b, head_mask=hm)
        assert float((g - r).abs().max()) <= 1e-3 and float((r - ref).abs().max()) > 1e-5, (B, L)
    with pytest.raises(_lib.MagbertError):
        eval_logits(m, weights.synthetic_bert_batch(2, 257, 47, 74, seed=1))


# ------------------------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("H", NEW)
def test_bf16_two_layers_vs_oracle(H):
    """test_model_gpu's bf16 bounds at 2 layers: logits 1e-2, gradients 3e-2 relative Frobenius, MAG's gated tensors 1e-1"""
    m = make(H, 2, torch.bfloat16).train()
    o = oracle(H, 2).train()
    b = weights.synthetic_bert_batch(4, 50, 47, 74, seed=21)
    ids, vis, aco, mask, seg, lab = tb(b, DEV)
    logits = m(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None)[0]
    torch.nn.MSELoss()(logits.view(-1), lab.view(-1)).backward()
    i2, v2, a2, m2, s2, l2 = tb(b)
    lo = o(i2, v2, a2, m2, s2)[0]
    torch.nn.functional.mse_loss(lo.view(-1), l2.view(-1)).backward()
    torch.cuda.synchronize()
    err = float((logits.detach().float().cpu() - lo.detach()).abs().max())
    print("bf16 H=%d 2 layers: logits max|err| %.3e" % (H, err))
    assert err <= 1e-2
    _grad_report(m, o, 3e-2, frobenius=True, loose=LOOSE_BF16, tol_loose=1e-1, show=4)


def _autocast_error(o, b):
    i2, v2, a2, m2, s2, _ = tb(b)
    with torch.no_grad():
        exact = o(i2, v2, a2, m2, s2)[0]
        with torch.autocast("cpu", torch.bfloat16):
            low = o(i2, v2, a2, m2, s2)[0]
    return float((low.float() - exact).abs().max()), exact


@pytest.mark.parametrize("H", NEW)
def test_bf16_full_depth_logits(golden, H):
    """bound = 2e-2 (the project's bound of the benchmarked 12 x 768 bf16 step) x max(1, a / b): a = the fp32 oracle's bf16-autocast error
    at this size and full depth, b = its autocast error at 12 x 768, same batch -- a ratio that comes from the reference alone"""
    B, L, V, seed = CASES[0]
    b = weights.synthetic_bert_batch(B, L, V, 74, seed=seed)
    a_err, exact = _autocast_error(oracle(H, None, V).eval(), b)
    b_err, _ = _autocast_error(oracle(768, None, V).eval(), b)
    bound = 2e-2 * max(1.0, a_err / b_err)
    m = make(H, None, torch.bfloat16, V, p_mag=0.5).eval()
    got = eval_logits(m, b)
    err = float(np.abs(got.numpy() - golden["g11_bert_sizes"][key("logits", H, B, L, V, seed)]).max())
    print("bf16 H=%d full depth: logits max|err| %.3e ; oracle autocast error %.3e at this size, %.3e at 12 x 768 -> bound %.3e" % (H, err, a_err, b_err, bound))
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------ the single-call step
def _steps(H, layers, cdt, graph, shapes=((4, 50),), nsteps=3, lr=1e-3, hidden_p=0.0, attn_p=0.0, p_mag=0.0, seed0=50):
    from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
    torch.manual_seed(77)
    m = make(H, layers, cdt, hidden_p=hidden_p, attn_p=attn_p, p_mag=p_mag).train()
    opt = AdamW(optimizer_grouped_parameters(m), lr=lr)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    losses, batches = [], []
    with m.stream_scope():
        for s in range(nsteps):
            B, L = shapes[s % len(shapes)]
            batches.append(weights.synthetic_bert_batch(B, L, 47, 74, seed=seed0 + s))
            losses.append(float(m.train_step(*tb(batches[-1], DEV), optimizer=opt, graph=graph)))
            sch.step()
    torch.cuda.synchronize()
    core = m._core
    out = dict(model=m, opt=opt, sch=sch, losses=losses, batches=batches, stats=core.graph_stats(),
               skipped=int(core.lib.mb_bert_word_skip_updates(core.handle)))
    if nsteps:
        out.update(p=m.flat_params.clone(), m=core._adam_m.clone(), v=core._adam_v.clone(), shadow=core.shadow.clone(), g=m.flat_grads.clone())
    return out


def _same(a, b, what):
    for k in ("p", "m", "v", "shadow"):
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)
    assert float(a["g"].abs().max()) == 0.0 and float(b["g"].abs().max()) == 0.0


def test_three_graph_steps_track_the_oracle_at_1024_fp32():
    """train_step(graph=True) at H = 1024: fwd + bwd + fused HF-AdamW + linear warmup, 3 steps, dropout off (as
    test_model_gpu.test_three_optimizer_steps_track_the_oracle_fp32)"""
    H, layers = 1024, 2
    run = _steps(H, layers, torch.float32, True)
    m = run["model"]
    assert run["stats"][0] >= 1 and run["stats"][1] == 3
    o = oracle(H, layers).train()
    oo = O.AdamW(O.grouped_parameters(o), lr=1e-3)
    so = O.get_linear_schedule_with_warmup(oo, num_warmup_steps=1.0, num_training_steps=10)
    ref = []
    for b in run["batches"]:
        i2, v2, a2, m2, s2, l2 = tb(b)
        oo.zero_grad()
        loss = torch.nn.functional.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1))
        ref.append(float(loss.detach()))
        loss.backward()
        oo.step(); so.step()
    assert float(m.flat_grads.abs().max()) == 0.0
    om = dict(o.named_parameters())
    worst = max(float((p.detach().cpu() - om[n].detach()).abs().max()) for n, p in m.named_parameters())
    print("H=1024 graph steps: losses %s oracle %s ; max |param - oracle param| %.3e" % (run["losses"], ref, worst))
    for a, r in zip(run["losses"], ref):
        assert abs(a - r) <= 1e-3 * max(1.0, abs(r))
    assert worst <= 2e-4
    m.eval(); o.eval()
    b = weights.synthetic_bert_batch(4, 50, 47, 74, seed=60)
    assert float((eval_logits(m, b) - oracle_logits(o, b)).abs().max()) <= 5e-3


def test_graph_step_equals_launch_by_launch_at_1024(monkeypatch):
    """deterministic mode, bf16, dropout on, two shapes: the replayed graph ends every step with the bits of the same launches one by one"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    kw = dict(shapes=((8, 50), (5, 40)), nsteps=4, hidden_p=0.1, attn_p=0.1, p_mag=0.5)
    g = _steps(1024, 2, torch.bfloat16, True, **kw)
    e = _steps(1024, 2, torch.bfloat16, "launches", **kw)
    assert g["stats"] == (2, 4) and e["stats"] == (0, 0), (g["stats"], e["stats"])
    _same(g, e, "graph vs launches")
    assert max(abs(a - b) for a, b in zip(g["losses"], e["losses"])) <= 2e-3


def test_word_row_skipping_sweep_equals_the_full_sweep_at_1024(monkeypatch):
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    kw = dict(shapes=((8, 50),), nsteps=3, hidden_p=0.1, attn_p=0.1, p_mag=0.5)
    monkeypatch.setenv("MB_ADAMW_SKIP_ZERO_ROWS", "0")
    off = _steps(1024, 2, torch.bfloat16, True, **kw)
    monkeypatch.setenv("MB_ADAMW_SKIP_ZERO_ROWS", "1")
    on = _steps(1024, 2, torch.bfloat16, True, **kw)
    assert off["skipped"] == 0 and on["skipped"] == 2, (off["skipped"], on["skipped"])      # (the first update has no proof yet)
    _same(on, off, "word-row skipping on vs off")


def test_attention_rider_override_on_an_fp32_engine_skips_nothing(monkeypatch):
    """MB_ADAMW_RIDE_ATTN_BLOCKS on an fp32 engine (no rider kernel: zero free slots): the override must not hand out a slice of the
    update that no launch runs"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    ref = _steps(1024, 3, torch.float32, True, shapes=((8, 50),), nsteps=2)
    monkeypatch.setenv("MB_ADAMW_RIDE_ATTN_BLOCKS", "64")
    got = _steps(1024, 3, torch.float32, True, shapes=((8, 50),), nsteps=2)
    for k in ("p", "m", "v"):
        assert torch.equal(ref[k], got[k]), k
    assert float(got["g"].abs().max()) == 0.0


_WORKER = r'''
import os, sys, torch
sys.path.insert(0, os.environ["REPO_ROOT"]); sys.path.insert(0, os.path.join(os.environ["REPO_ROOT"], "tests"))
import torch.distributed as dist
from test_bert_sizes_gpu import _steps, make, tb, weights, DEV
job = os.environ["JOB"]
if job == "ride":
    r = _steps(1024, 4, torch.bfloat16, True, shapes=((48, 50),), nsteps=3, hidden_p=0.1, attn_p=0.1, p_mag=0.5)
    torch.save({k: r[k].cpu() for k in ("p", "m", "v", "shadow", "g")}, os.environ["OUT"])
else:                                  # the one-rank RCCL data-parallel step (or the plain one), 6 layers
    from bert_multimodal_transformer_amd import AdamW, get_linear_schedule_with_warmup
    from bert_multimodal_transformer_amd.distributed import DataParallel
    from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
    torch.cuda.set_device(0)
    use_dp = os.environ["USE_DP"] == "1"
    if use_dp:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    m = make(1024, 6, torch.float32).train()
    opt = AdamW(optimizer_grouped_parameters(m), lr=1e-3)
    sch = get_linear_schedule_with_warmup(opt, 0, 100)
    dp = None
    if use_dp:
        dp = DataParallel(m, opt)
        dp.broadcast_parameters(0)
    with m.stream_scope():
        for s in range(3):
            m.train_step(*tb(weights.synthetic_bert_batch(8, 50, 47, 74, seed=90 + s), DEV), optimizer=opt, graph=None)
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


def test_riders_change_nothing_at_1024(tmp_path):
    """MB_DETERMINISTIC=1, bf16, 4 layers, B = 48, L = 50 (T = 2,400): with riders on, launches of the step really carry pieces of the
    AdamW update (the engine's "[magbert ride] params=" lines under MB_GEMM_LOG=1) and the step ends with the bits of the run without"""
    common = dict(JOB="ride", MB_DETERMINISTIC="1", MB_GEMM_LOG="1")
    off, log_off = _worker(tmp_path, "off.pt", dict(common, MB_ADAMW_RIDE="0"))
    on, log_on = _worker(tmp_path, "on.pt", dict(common, MB_ADAMW_RIDE="1"))
    ridden = [int(l.split("params=")[1].split()[0]) for l in log_on.splitlines() if l.startswith("[magbert ride] params=")]
    print("H=1024 riders: %d launches carried %d parameters (first graph capture)" % (len(ridden), sum(ridden)))
    assert len(ridden) > 0 and sum(ridden) > 0, log_on[-2000:]
    assert not [l for l in log_off.splitlines() if l.startswith("[magbert ride] params=")]
    for k in ("p", "m", "v", "shadow"):
        assert torch.equal(on[k], off[k]), k
    assert float(on["g"].abs().max()) == 0.0


def test_single_call_dp_step_over_rccl_one_rank_at_1024(tmp_path):
    """mb_bert_train_step_dp at H = 1024 with 6 layers -- pieces of 2 | 2 | 2 layers, not the 4 | 4 | 2 | 2 of the 12-layer model -- over a
    one-rank RCCL communicator: every collective is an identity, so in deterministic mode fp32 parameters after three steps are
    bit-identical to the plain single-call step (the rule of test_dp_gpu.test_single_call_dp_step_over_rccl_one_rank)"""
    from conftest import free_port
    common = dict(JOB="dp", MB_DETERMINISTIC="1", MB_DP_FORCE="1", MB_DP_GRAD_DTYPE="fp32", RANK="0", WORLD_SIZE="1",
                  MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    a, _ = _worker(tmp_path, "plain.pt", dict(common, USE_DP="0", MASTER_PORT=str(free_port())))
    b, _ = _worker(tmp_path, "dp.pt", dict(common, USE_DP="1", MASTER_PORT=str(free_port())))
    assert b["fused"] and not a["fused"]
    print("H=1024 6 layers, one-rank RCCL: %d collectives, %.1f MB; max |dparam| %.3e" % (b["stats"][0], b["stats"][1] * 1e-6,
                                                                                         float((a["p"] - b["p"]).abs().max())))
    assert b["stats"][0] >= 3
    assert torch.equal(a["p"], b["p"])


# ------------------------------------------------------------------------------------------------------------ checkpoint, driver
def test_checkpoint_of_a_large_model_resumes_bit_equal(tmp_path, monkeypatch):
    """bert-large (24 x 1024): state_dict + optimizer state + dropout counter after 2 steps into fresh objects: step 3 is bit-equal to
    the uninterrupted run (deterministic mode, bf16, dropout on)"""
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    kw = dict(shapes=((8, 50),), hidden_p=0.1, attn_p=0.1, p_mag=0.5)
    run = _steps(1024, None, torch.bfloat16, True, nsteps=2, **kw)
    m, opt, sch = run["model"], run["opt"], run["sch"]
    path = str(tmp_path / "ckpt.pt")
    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}, "opt": opt.state_dict(), "sch": sch.state_dict(),
                "rng": m.get_rng_state()}, path)
    b3 = weights.synthetic_bert_batch(8, 50, 47, 74, seed=52)
    m.train_step(*tb(b3, DEV), optimizer=opt, graph=True)
    torch.cuda.synchronize()
    want = (m.flat_params.clone(), m._core._adam_m.clone(), m._core._adam_v.clone())
    del run, m, opt, sch
    torch.cuda.empty_cache()
    fresh = _steps(1024, None, torch.bfloat16, True, nsteps=0, **kw)
    m2, opt2, sch2 = fresh["model"], fresh["opt"], fresh["sch"]
    ck = torch.load(path)
    m2.load_state_dict(ck["model"]); opt2.load_state_dict(ck["opt"]); sch2.load_state_dict(ck["sch"]); m2.set_rng_state(ck["rng"])
    m2.train_step(*tb(b3, DEV), optimizer=opt2, graph=True)
    torch.cuda.synchronize()
    for x, y in zip(want, (m2.flat_params, m2._core._adam_m, m2._core._adam_v)):
        assert torch.equal(x, y)


def test_from_pretrained_reads_the_config_json_of_a_large_checkpoint(tmp_path):
    import json
    src = make(1024, 2, torch.float32)
    torch.save({k: v.cpu() for k, v in src.state_dict().items() if k.startswith("bert.")}, tmp_path / "pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps(dict(size_config(1024, 2), model_type="bert", vocab_size=30522, architectures=["BertModel"])))
    p = MAG_BertForSequenceClassification.from_pretrained(str(tmp_path), multimodal_config=MultimodalConfig(1.0, 0.0), visual_dim=47, acoustic_dim=74)
    assert (p.config.hidden_size, p.config.num_attention_heads, p.config.num_hidden_layers) == (1024, 16, 2)
    assert sorted(k for k in p.loading_info["missing_keys"] if not k.startswith(("bert.MAG.", "classifier."))) == []
    for k, v in src.state_dict().items():
        if k.startswith("bert.") and not k.startswith("bert.MAG."):
            assert torch.equal(p.state_dict()[k], v), k


def test_driver_runs_bert_large():
    r = subprocess.run([sys.executable, "-m", "bert_multimodal_transformer_amd.multimodal_driver", "--model", "bert-large-uncased",
                        "--synthetic", "1284", "--n_epochs", "1"], cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import re
    losses = [float(x) for x in re.findall(r"train_loss[:=]\s*([-+0-9.eE]+|nan|inf)", r.stdout)]
    assert "nan" not in r.stdout.lower() and all(np.isfinite(losses)), r.stdout[-2000:]
