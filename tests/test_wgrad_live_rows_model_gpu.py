"""GPU: the single-call MAG-BERT step with its layers' weight gradients summed over the live token rows only (MB_WGRAD_LIVE_ROWS,
csrc/engine_common.h StepMixin::live_built) against the same step with dense sums (MB_WGRAD_LIVE_ROWS=0).

A 2 x 256 model, B = 4, L = 50, bf16, MB_DETERMINISTIC=1, one step without optimizer (the gradients stay in the flat buffer):
  * a batch of mixed lengths with one fully padded sample: every gradient that is not a layer's GEMM weight has the same bits in both
    modes; a layer's GEMM weight gradients differ by a regrouping of the same exact products at most -- per element
    2 * Tp 2^-24 (|dY|^T |X|) + 2 * 2^-24 |g|: each of the two fp32 sums of at most Tp products is within Tp 2^-24 |dY|^T |X| of the exact
    sum (any order), and each store rounds once.  |dY|^T |X| is formed in fp64 from the operands the dense step left in the workspace;
  * the rows the list leaves out really are zero in every dY operand of both layers (a -0.0 counts as zero: it adds nothing), and the
    dense step's rows of a fully padded sample are NOT all zero -- which is why the list keeps such a sample whole;
  * sample 3 has live tokens behind a [CLS] row whose own mask word is 0: that row is a query like any other and the head reads it, so
    its dY is NOT zero (asserted, in every layer) and the list must hold it;
  * mode 2 (the [CLS]-row list for the top layer's ffn2 / ffn1 / out-proj problems): those dY are zero off the [CLS] rows;
  * an all-live batch: the same bits in all three modes.
Every step also asserts how many weight-gradient launches summed over a list (mb_bert_debug_live_wgrad_launches): one per layer in modes
1 and 2, none in mode 0 -- a step that fell back to dense would pass every comparison above for nothing.
Deterministic mode runs the dense sums unless MB_WGRAD_LIVE_ROWS asks for a list by name (it promises the bits of the python-driven
passes), so the mode is set explicitly here."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import BertConfig, MAG_BertForSequenceClassification, MultimodalConfig
from oracle import weights

DEV = "cuda:0"
B, L, HID, NLAYER = 4, 50, 256, 2
WNAMES = ("attention.self.query.weight", "attention.self.key.weight", "attention.self.value.weight", "attention.output.dense.weight",
          "intermediate.dense.weight", "output.dense.weight")


def _batch(kind):
    b = weights.synthetic_bert_batch(B, L, 47, 74, seed=31)
    if kind == "all_live":
        b["input_mask"][:] = 1
    else:
        lens = [50, 7, 0, 23]                      # sample 0 full, sample 2 all padding
        for i, n in enumerate(lens):
            b["input_mask"][i, :] = 0
            b["input_mask"][i, :n] = 1
        b["input_mask"][3, 0] = 0                  # sample 3: 22 live tokens, the [CLS] row's own mask word is 0
        b["input_ids"][2, :] = 0
        b["visual"][2] = 0
        b["acoustic"][2] = 0
    return b


def _operand(core, layer, which, rows):
    ld = C.c_int(0)
    ptr = core.lib.mb_bert_debug_wgrad_dy(core.handle, layer, which, C.byref(ld))
    assert ptr
    off = ptr - core.ws.data_ptr()
    return core.ws[off: off + rows * ld.value * 2].view(torch.bfloat16).view(rows, ld.value).clone()


def _step(monkeypatch, mode, kind):
    monkeypatch.setenv("MB_DETERMINISTIC", "1")
    monkeypatch.setenv("MB_WGRAD_LIVE_ROWS", mode)
    torch.manual_seed(5)
    cfg = BertConfig(hidden_size=HID, num_hidden_layers=NLAYER, num_attention_heads=4, intermediate_size=4 * HID, num_labels=1,
                     hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    m = MAG_BertForSequenceClassification(cfg, MultimodalConfig(1.0, 0.5), visual_dim=47, acoustic_dim=74, compute_dtype=torch.bfloat16)
    m.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(p.shape), "test")) for n, p in m.named_parameters()})
    m.train()
    b = _batch(kind)
    t = lambda k: torch.from_numpy(b[k]).to(DEV)
    with m.stream_scope():
        m.train_step(t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"), t("label_ids"), optimizer=None, graph=True)
    torch.cuda.synchronize()
    core = m._core
    assert int(core.lib.mb_bert_debug_live_wgrad_launches(core.handle)) == (0 if mode == "0" else NLAYER), "mode %s: not the launches asked for" % mode
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    ops = {(l, w): _operand(core, l, w, B * L) for l in range(NLAYER) for w in range(8)}
    return grads, ops, b["input_mask"].copy()


def _is_layer_weight(name):
    return name.startswith("bert.encoder.layer.") and name.endswith(WNAMES)


def test_mixed_lengths(monkeypatch):
    g0, ops0, mask = _step(monkeypatch, "0", "mixed")
    g1, ops1, _ = _step(monkeypatch, "1", "mixed")
    g2, ops2, _ = _step(monkeypatch, "2", "mixed")
    real = mask.any(axis=1)
    lm = (mask != 0) | ~real[:, None]
    lm[:, 0] = True                                # the [CLS] row of every sample
    live = torch.from_numpy(lm.reshape(-1))
    assert int(live.sum()) == 50 + 7 + 50 + 23
    cls = torch.zeros(B * L, dtype=torch.bool)
    cls[::L] = True
    # the [CLS] row of sample 3 (mask word 0, live tokens behind it) carries a gradient in every layer: ffn2, ffn1, out-proj dY and the Q
    # third of dqkv
    for l in range(NLAYER):
        for w in range(3):
            assert float(ops0[(l, w)][3 * L].float().abs().max()) > 0.0, "layer %d dY %d: the masked [CLS] row is zero" % (l, w)
        assert float(ops0[(l, 3)][3 * L, :HID].float().abs().max()) > 0.0, "layer %d dQ: the masked [CLS] row is zero" % l
    # the top layer's ffn2 / ffn1 / out-proj dY are zero off the [CLS] rows (what mode 2 relies on)
    for w in range(3):
        assert float(ops0[(NLAYER - 1, w)][~cls].float().abs().max()) == 0.0, "top layer dY %d is non-zero off the [CLS] rows" % w
    # the rows the list leaves out are zero in every dY operand, in all modes
    for ops, what in ((ops0, "dense"), (ops1, "live rows"), (ops2, "live + cls rows")):
        for l in range(NLAYER):
            for w in range(4):
                dead = ops[(l, w)][~live].float()
                assert float(dead.abs().max()) == 0.0, "%s: layer %d dY %d has a non-zero padding row" % (what, l, w)
            for w in range(4, 8):
                assert bool(torch.isfinite(ops[(l, w)].float()).all()), "%s: layer %d X %d is not finite" % (what, l, w)
    # ... and a fully padded sample is no such row: its rows carry a gradient
    assert float(ops0[(NLAYER - 1, 0)][2 * L].float().abs().max()) > 0.0
    assert float(ops0[(0, 3)][2 * L:3 * L].float().abs().max()) > 0.0
    Tp = -(-B * L // 64) * 64
    # the six parameters of a layer are the four GEMMs' outputs: query | key | value are row blocks of the fused qkv problem
    prob_of = {WNAMES[0]: (3, 0), WNAMES[1]: (3, 1), WNAMES[2]: (3, 2), WNAMES[3]: (2, 0), WNAMES[4]: (1, 0), WNAMES[5]: (0, 0)}
    for n in g0:
        if not _is_layer_weight(n):
            for g in (g1, g2):
                assert torch.equal(g0[n].view(torch.int32), g[n].view(torch.int32)), n + ": differs, and is no gathered weight gradient"
            continue
        l = int(n.split(".")[3])
        which, blk = prob_of[n[len("bert.encoder.layer.%d." % l):]]
        dY, X = ops0[(l, which)].double().abs(), ops0[(l, which + 4)].double().abs()
        rows = g0[n].shape[0]
        S = dY[:, blk * rows:(blk + 1) * rows].t() @ X[:, :g0[n].shape[1]]
        bound = 2 * Tp * 2.0 ** -24 * S + 2 * 2.0 ** -24 * g0[n].double().abs() + 1e-30
        for mode, g in (("1", g1), ("2", g2)):
            ratio = float(((g[n].double() - g0[n].double()).abs() / bound).max())
            print("mode %s %s: worst |diff| / bound %.3f" % (mode, n, ratio))
            assert ratio <= 1.0, "mode %s %s: |diff| / bound %.3f" % (mode, n, ratio)
        assert float(g0[n].abs().max()) > 0.0


def test_all_live_is_bit_identical(monkeypatch):
    g0, _, _ = _step(monkeypatch, "0", "all_live")
    g1, _, _ = _step(monkeypatch, "1", "all_live")
    g2, _, _ = _step(monkeypatch, "2", "all_live")
    for n in g0:
        assert torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)), n + ": mode 1 differs on an all-live batch"
    # (mode 2 sums the top layer's three problems over fewer rows: another grouping of the same products there, the same bits elsewhere)
    for n in g0:
        if not (_is_layer_weight(n) and n.startswith("bert.encoder.layer.%d." % (NLAYER - 1)) and "self" not in n):
            assert torch.equal(g0[n].view(torch.int32), g2[n].view(torch.int32)), n + ": mode 2 differs on an all-live batch"
