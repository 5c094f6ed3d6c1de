"""CPU: MAG-XLNet at d_model 256, 512, 768 and 1024 (xlnet-large-cased) -- the engine's gate, parameter layout and workspace sizes, the
fixture tests/golden/g12_xlnet_sizes.npz against the oracle, the Python surface (XLNetConfig, config.json, the driver) and step_bench's
flags.  No GPU needed."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from bert_multimodal_transformer_amd import MAG_XLNetForSequenceClassification, MAG_XLNetModel, MultimodalConfig, XLNetConfig, _lib
from bert_multimodal_transformer_amd import xlnet as mb_xlnet
from oracle import mag_xlnet_ref as X, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_xlnet_sizes import (CASES, EXTRA_H, EXTRA_LAYERS, MEMS_CASE, QS_CASE, SAMPLE, SIZES, key, query_stream_inputs,      # noqa: E402
                                     size_config)

MB_ERR_SHAPE, MB_ERR_ARG = 1001, 1000
BASE = (768, 12, 3072, 12)


def _cfg(H, nh, inner, layers, dtype=_lib.DT_BF16, max_batch=4, max_seq=128, labels=1, inj=None):
    return _lib.XlnetEngineConfig(32000, H, layers, nh, inner, labels, 47, 74, min(1, layers - 1) if inj is None else inj, 1e-12, 1e-5, 1.0,
                                  0.1, 0.1, 0.5, dtype, max_batch, max_seq)


def _create(cfg):
    h = C.c_void_p()
    rc = _lib.lib().mb_xlnet_create(C.byref(cfg), C.byref(h))
    return rc, h


def _table(h):
    """[(name, offset, numel, shape, decay)] of an engine"""
    L = _lib.lib()
    rows = []
    for i in range(L.mb_xlnet_num_tensors(h)):
        name = C.create_string_buffer(160)
        off, numel, ndim, dec = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
        shp = (C.c_int64 * 4)()
        assert L.mb_xlnet_tensor_info(h, i, name, 160, C.byref(off), C.byref(numel), C.byref(ndim), shp, C.byref(dec)) == 0
        rows.append((name.value.decode(), off.value, numel.value, tuple(shp[k] for k in range(ndim.value)), dec.value))
    return rows


def test_error_codes_are_the_librarys():
    assert "shape" in _lib.lib().mb_error_string(MB_ERR_SHAPE).decode().lower()


def test_engine_accepts_the_four_widths_and_refuses_the_rest():
    L = _lib.lib()
    counts = {}
    for (H, nh, inner, layers) in SIZES + (BASE,):
        for dt in (_lib.DT_BF16, _lib.DT_F32):
            for max_seq in (128, 256):                              # 256: the tiled relative attention's workspace (stats, two planes, 128-row psave)
                rc, h = _create(_cfg(H, nh, inner, layers, dt, max_seq=max_seq))
                assert rc == 0, (H, dt, max_seq)
                counts[H] = L.mb_xlnet_param_count(h)
                assert L.mb_xlnet_workspace_bytes(h) > 0
                L.mb_xlnet_destroy(h)
    assert counts[256] < counts[512] < counts[768] < counts[1024]
    assert 362e6 < counts[1024] < 365e6                           # xlnet-large 360.3 M + MAG 2.3 M + summary 1.05 M + head, alignment included
    assert _create(_cfg(384, 6, 1536, 2))[0] == MB_ERR_SHAPE     # not one of the four
    assert _create(_cfg(640, 10, 2560, 2))[0] == MB_ERR_SHAPE
    assert _create(_cfg(1280, 20, 5120, 2))[0] == MB_ERR_SHAPE
    assert _create(_cfg(1024, 12, 4096, 2))[0] == MB_ERR_SHAPE   # heads of 64 only
    assert _create(_cfg(256, 8, 1024, 2))[0] == MB_ERR_SHAPE
    assert _create(_cfg(1024, 16, 4096, 0, inj=0))[0] == MB_ERR_SHAPE   # at least one layer
    assert _create(_cfg(1024, 16, 4000, 2))[0] == MB_ERR_SHAPE   # d_inner % 128, as before
    assert _create(_cfg(1024, 16, 4096, 2, inj=2))[0] != 0       # the injection layer must exist
    for layers in (1, 5, 30, 40):                                 # any depth (above 31 the LayerNorm reductions go layer by layer)
        rc, h = _create(_cfg(256, 4, 1024, layers))
        assert rc == 0, layers
        L.mb_xlnet_destroy(h)


def test_large_parameter_table_is_the_oracles_state_dict():
    L = _lib.lib()
    H, nh, inner, layers = SIZES[0]
    rc, h = _create(_cfg(H, nh, inner, layers))
    assert rc == 0
    rows = _table(h)
    with torch.device("meta"):
        o = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**size_config(H)), X.MultimodalConfig(1.0, 0.5), 47, 74)
    want = {k: tuple(v.shape) for k, v in o.state_dict().items()}
    got = {r[0]: r[3] for r in rows}
    assert got == want
    nd, n, nt = L.mb_xlnet_decay_count(h), L.mb_xlnet_param_count(h), L.mb_xlnet_trainable_count(h)
    end = 0
    for name, off, numel, shape, dec in sorted(rows, key=lambda r: r[1]):
        assert off % 64 == 0 and off >= end and numel == int(np.prod(shape)), name
        end = off + numel
        assert (off + numel <= nd) if dec == 1 else (nd <= off and (off + numel <= nt if dec == 0 else off >= nt)), name
    assert end <= n and nd % 64 == 0
    b, e = C.c_size_t(), C.c_size_t()
    L.mb_xlnet_shadow_range(h, C.byref(b), C.byref(e))
    per_layer = 5 * H * H + 2 * H * inner
    assert b.value == 0 and e.value == layers * per_layer + H * H          # every layer's GEMM weights + the summary, contiguous
    # q | k | v of a layer lie next to each other, d_model * d_model apart: the fused N = 3 H projection reads them as one operand
    off = {r[0]: r[1] for r in rows}
    for l in (0, layers - 1):
        q, k, v = (off["transformer.layer.%d.rel_attn.%s" % (l, t)] for t in "qkv")
        assert k - q == H * H and v - k == H * H
    # the backward stages' gradient ranges tile [0, trainable) at depth 24
    offs, lens = (C.c_size_t * 8)(), (C.c_size_t * 8)()
    spans = []
    for stage in range(layers + 2):
        k = L.mb_xlnet_stage_grad_ranges(h, stage, offs, lens, 8)
        assert k >= 1
        spans += [(offs[i], offs[i] + lens[i]) for i in range(k)]
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == nt and all(a[1] == b_[0] for a, b_ in zip(spans, spans[1:]))
    L.mb_xlnet_destroy(h)


@pytest.mark.parametrize("H,nh,inner,layers", SIZES + (BASE,))
def test_query_stream_scratch_sizes(H, nh, inner, layers):
    """mb_xlnet_query_stream_state_bytes / _scratch_bytes at n_head != 12: one state per layer boundary, rows padded to 128"""
    L = _lib.lib()
    for dt, es in ((_lib.DT_F32, 4), (_lib.DT_BF16, 2)):
        rc, h = _create(_cfg(H, nh, inner, 2, dt))
        assert rc == 0
        B, M, Lq = 4, 5, 50
        stride = L.mb_xlnet_query_stream_state_bytes(h, B, M)
        need = L.mb_xlnet_query_stream_scratch_bytes(h, B, M, Lq)
        R, T = 128, 256                                           # B * M = 20 and B * L = 200 rounded up to 128
        assert stride == R * H * es and stride % 256 == 0
        lower = 3 * stride + (R * H * 5 + T * H * 4 + R * inner * 2) * es
        assert lower <= need <= lower + 64 * 1024, (need, lower)
        L.mb_xlnet_destroy(h)


@pytest.mark.parametrize("H", [s[0] for s in SIZES])
def test_oracle_reproduces_the_reference_fixture(golden, H):
    g = golden["g12_xlnet_sizes"]
    o = {}
    for (B, L, V, seed) in CASES:
        if V not in o:
            m = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**size_config(H)), X.MultimodalConfig(1.0, 0.5), V, 74)
            o[V] = X.load_deterministic(m, "test").eval()
        b = weights.synthetic_xlnet_batch(B, L, V, 74, seed=seed)
        t = lambda k: torch.from_numpy(b[k])
        with torch.no_grad():
            logits = o[V](t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"))[0]
            seq = o[V].transformer(t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"))
        ref = g[key("logits", H, B, L, V, seed)]
        assert ref.shape == (B, 1)
        assert float(np.abs(logits.numpy() - ref).max()) <= 2e-5
        assert float(np.abs(weights.strided_sample(seq.numpy(), SAMPLE) - g[key("seq", H, B, L, V, seed)]).max()) <= 2e-5


def test_oracle_reproduces_the_mems_and_query_stream_entries(golden):
    g = golden["g12_xlnet_sizes"]
    H = EXTRA_H
    o = X.load_deterministic(X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**size_config(H, EXTRA_LAYERS)),
                                                                  X.MultimodalConfig(1.0, 0.5), 47, 74), "test").eval()
    tb = lambda b: tuple(torch.from_numpy(b[k]) for k in ("input_ids", "visual", "acoustic", "input_mask", "segment_ids"))
    B, L, ml, seed = MEMS_CASE
    tag = "H%d/B%d_L%d_M%d_seed%d" % (H, B, L, ml, seed)
    with torch.no_grad():
        l1 = o(*tb(weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed)), mem_len=ml)[0]
        mems1 = o.transformer.new_mems
        l2 = o(*tb(weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed + 100)), mems=mems1, mem_len=ml)[0]
        mems2 = o.transformer.new_mems
    assert float(np.abs(l1.numpy() - g["mems/logits_seg1/" + tag]).max()) <= 2e-5
    assert float(np.abs(l2.numpy() - g["mems/logits_seg2/" + tag]).max()) <= 2e-5
    assert tuple(mems2[0].shape) == (ml, B, H)
    for i in range(EXTRA_LAYERS):
        for name, mm in (("seg1", mems1), ("seg2", mems2)):
            ref = g["mems/new_mems_%s/%s/layer%d" % (name, tag, i)]
            assert float(np.abs(weights.strided_sample(mm[i].numpy(), SAMPLE) - ref).max()) <= 2e-5
    B, L, M, seed = QS_CASE
    tag = "H%d/B%d_L%d_M%d_seed%d" % (H, B, L, M, seed)
    b = weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed)
    tm, pm = query_stream_inputs(b["input_mask"], M, seed)
    assert tm.shape == (B, M, L) and float(tm.sum()) == B * M and pm.shape == (B, L, L)
    with torch.no_grad():
        og = o.transformer(*tb(b), perm_mask=torch.from_numpy(pm), target_mapping=torch.from_numpy(tm))
        lg = o(*tb(b), perm_mask=torch.from_numpy(pm), target_mapping=torch.from_numpy(tm))[0]
    assert tuple(og.shape) == (B, M, H)
    assert float(np.abs(weights.strided_sample(og.numpy(), SAMPLE) - g["qs/output_g/" + tag]).max()) <= 2e-5
    assert float(np.abs(lg.numpy() - g["qs/logits/" + tag]).max()) <= 2e-5


def test_fixture_is_small_and_complete(golden):
    g = golden["g12_xlnet_sizes"]
    want = [key(k, s[0], *c) for k in ("logits", "seq") for s in SIZES for c in CASES]
    mt = "H%d/B%d_L%d_M%d_seed%d" % ((EXTRA_H,) + MEMS_CASE)
    qt = "H%d/B%d_L%d_M%d_seed%d" % ((EXTRA_H,) + QS_CASE)
    want += ["mems/logits_seg1/" + mt, "mems/logits_seg2/" + mt, "qs/output_g/" + qt, "qs/logits/" + qt]
    want += ["mems/new_mems_%s/%s/layer%d" % (s, mt, i) for s in ("seg1", "seg2") for i in range(EXTRA_LAYERS)]
    assert sorted(g.files) == sorted(want)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g12_xlnet_sizes.npz")) < 16 * 1024


def test_config_size_check_names_the_supported_set():
    bad = (dict(d_model=384, n_head=6, d_inner=1536), dict(d_model=640, n_head=10, d_inner=2560),      # not one of the four
           dict(d_model=1024, n_head=12, d_inner=4096),                                                # heads of 64 only
           dict(d_model=1024, n_head=16, d_inner=4000),                                                # d_inner % 128
           dict(d_model=256, n_head=4, d_inner=1024, n_layer=0))                                       # at least one layer
    for kw in bad:
        with pytest.raises(ValueError) as ei:
            mb_xlnet.check_xlnet_sizes(XLNetConfig(**kw))
        assert all(s in str(ei.value) for s in ("256", "512", "768", "1024")), str(ei.value)
        for cls in (MAG_XLNetForSequenceClassification, MAG_XLNetModel):      # the constructors say the same, before they look for a device
            with pytest.raises(ValueError) as ei:
                cls(XLNetConfig(**kw), MultimodalConfig(1.0, 0.5))
            assert "256, 512, 768, 1024" in str(ei.value)
    for (H, nh, inner, layers) in SIZES:
        mb_xlnet.check_xlnet_sizes(XLNetConfig(**size_config(H)), 1)
    mb_xlnet.check_xlnet_sizes(XLNetConfig(), 1)
    c = XLNetConfig.large(num_labels=3)
    assert (c.d_model, c.n_head, c.n_layer, c.d_inner, c.num_labels, c.d_head) == (1024, 16, 24, 4096, 3, 64)
    assert "1024" in XLNetConfig.__doc__ and "xlnet-large" in XLNetConfig.__doc__


def test_injection_index_beyond_the_last_layer_raises_by_name():
    for inj in (2, 5, -1):
        with pytest.raises(ValueError) as ei:
            MAG_XLNetForSequenceClassification(XLNetConfig(n_layer=2), MultimodalConfig(1.0, 0.5), injection_index=inj)
        assert "injection_index" in str(ei.value) and "n_layer" in str(ei.value)
    mb_xlnet.check_xlnet_sizes(XLNetConfig(n_layer=2), 1)
    mb_xlnet.check_xlnet_sizes(XLNetConfig(n_layer=1), 0)


def test_config_json_beside_a_checkpoint_selects_the_model_size(tmp_path):
    """what from_pretrained does without config=: the directory's config.json (only the keys XLNetConfig knows) -> the engine's parameter
    table for that configuration takes the state dict saved from the oracle of the same size"""
    H, nh, inner, layers = SIZES[2]
    o = X.load_deterministic(X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**size_config(H)), X.MultimodalConfig(1.0, 0.5), 47, 74), "test")
    torch.save(o.state_dict(), tmp_path / "pytorch_model.bin")
    hf = {"architectures": ["XLNetLMHeadModel"], "model_type": "xlnet", "untie_r": True, "d_head": 64, "bos_token_id": 1, "pad_token_id": 5,
          "task_specific_params": {"text-generation": {"do_sample": True, "max_length": 250}}, "start_n_top": 5, "end_n_top": 5,
          "d_model": H, "n_head": nh, "d_inner": inner, "n_layer": layers, "vocab_size": 32000, "ff_activation": "gelu", "attn_type": "bi",
          "bi_data": False, "clamp_len": -1, "mem_len": None, "reuse_len": None, "same_length": False, "dropout": 0.1,
          "initializer_range": 0.02, "layer_norm_eps": 1e-12, "summary_type": "last", "summary_use_proj": True, "summary_activation": "tanh",
          "summary_last_dropout": 0.1}
    (tmp_path / "config.json").write_text(json.dumps(hf))
    for where in (str(tmp_path), str(tmp_path / "pytorch_model.bin")):
        c = mb_xlnet.read_xlnet_config_beside(where, num_labels=1)
        assert (c.d_model, c.n_head, c.d_inner, c.n_layer, c.num_labels) == (H, nh, inner, layers, 1)
        assert not hasattr(c, "architectures") and not hasattr(c, "untie_r")
    for cls in (MAG_XLNetForSequenceClassification, MAG_XLNetModel):
        assert cls._config_beside(str(tmp_path), 1).d_model == H
    rc, h = _create(_cfg(c.d_model, c.n_head, c.d_inner, c.n_layer))
    assert rc == 0
    got = {r[0]: r[3] for r in _table(h)}
    _lib.lib().mb_xlnet_destroy(h)
    sd = torch.load(tmp_path / "pytorch_model.bin", map_location="cpu")
    assert got == {k: tuple(v.shape) for k, v in sd.items()}
    # a config.json of another model family, or none at all: xlnet-base stays the default
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "bert", "hidden_size": 1024, "num_attention_heads": 16}))
    assert mb_xlnet.read_xlnet_config_beside(str(tmp_path)) is None
    os.remove(tmp_path / "config.json")
    assert mb_xlnet.read_xlnet_config_beside(str(tmp_path)) is None
    assert MAG_XLNetForSequenceClassification._config_beside(str(tmp_path), 1) is None
    d = MAG_XLNetForSequenceClassification._default_config(1)
    assert (d.d_model, d.n_layer) == (768, 12)


def test_driver_knows_xlnet_large():
    from bert_multimodal_transformer_amd import multimodal_driver as D
    a = D.parse_args(["--model", "xlnet-large-cased", "--synthetic", "8"])
    assert a.model == "xlnet-large-cased" and a.model in D.XLNET_MODELS and a.model not in D.BERT_MODELS
    c = D.xlnet_config(a.model)
    assert (c.d_model, c.n_head, c.n_layer, c.d_inner) == (1024, 16, 24, 4096)
    assert D.xlnet_config("xlnet-base-cased").d_model == 768
    with pytest.raises(SystemExit):
        D.parse_args(["--model", "xlnet-huge"])
    with pytest.raises((ValueError, RuntimeError)) as ei:          # (RuntimeError: no transformers tokenizers on this machine)
        D.get_tokenizer("gpt2")
    if isinstance(ei.value, ValueError):
        assert all(n in str(ei.value) for n in ("bert-base-uncased", "bert-large-uncased", "xlnet-base-cased", "xlnet-large-cased"))
    # the feature layout of an XLNet model: left padded, <sep> <cls> at the end, segment id 2 on <cls>
    old = getattr(D, "args", None)
    try:
        D.args = a
        D.args.max_seq_length = 8
        tok = type("T", (), {"cls_token": "<cls>", "sep_token": "<sep>", "pad_token_id": 5, "tokenize": lambda s, w: [w],
                             "convert_tokens_to_ids": lambda s, t: [7] * len(t)})()
        f = D.convert_to_features([((["a", "b"], np.ones((2, 47)), np.ones((2, 74))), 1.0, "s")], 8, tok)[0]
        assert f.input_mask == [0, 0, 0, 0, 1, 1, 1, 1] and f.segment_ids == [3, 3, 3, 3, 0, 0, 0, 2] and f.input_ids[:4] == [5] * 4
    finally:
        D.args = old


def test_step_bench_takes_the_size_flags_for_xlnet():
    src = open(os.path.join(ROOT, "tools", "step_bench.cpp")).read()
    assert "xc.d_model = hidden" in src and "xc.n_head = heads" in src and "xc.d_inner = inter" in src and "xc.n_layer = layers" in src
    assert "MAG-BERT only" not in src
    hdr = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    assert "xlnet-large-cased" in hdr and "the MAG-XLNet engine: 768" not in hdr
