"""CPU: MAG-BERT at hidden sizes 256, 512, 768 and 1024 (bert-large-uncased) -- the engine's gate and parameter layout, the fixture
tests/golden/g11_bert_sizes.npz against the oracle, the Python surface (BertConfig, config.json, the driver) and step_bench's flags.
No GPU needed."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from bert_multimodal_transformer_amd import BertConfig, MAG_BertForSequenceClassification, MultimodalConfig, _lib
from bert_multimodal_transformer_amd import bert as mb_bert
from oracle import mag_bert_ref as R, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_sizes import CASES, SAMPLE, SIZES, key, size_config      # noqa: E402

MB_ERR_SHAPE = 1001


def _cfg(H, nh, inter, layers, dtype=_lib.DT_BF16, max_batch=4, max_seq=128, labels=1):
    return _lib.BertEngineConfig(30522, H, layers, nh, inter, 512, 2, labels, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, dtype,
                                 max_batch, max_seq)


def _create(cfg):
    h = C.c_void_p()
    rc = _lib.lib().mb_bert_create(C.byref(cfg), C.byref(h))
    return rc, h


def _table(h):
    """[(name, offset, numel, shape, decay)] of an engine"""
    L = _lib.lib()
    rows = []
    for i in range(L.mb_bert_num_tensors(h)):
        name = C.create_string_buffer(160)
        off, numel, ndim, dec = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
        shp = (C.c_int64 * 4)()
        assert L.mb_bert_tensor_info(h, i, name, 160, C.byref(off), C.byref(numel), C.byref(ndim), shp, C.byref(dec)) == 0
        rows.append((name.value.decode(), off.value, numel.value, tuple(shp[k] for k in range(ndim.value)), dec.value))
    return rows


def test_engine_accepts_the_four_hidden_sizes_and_refuses_the_rest():
    L = _lib.lib()
    counts = {}
    for (H, nh, inter, layers) in SIZES + ((768, 12, 3072, 12),):
        for dt in (_lib.DT_BF16, _lib.DT_F32):
            rc, h = _create(_cfg(H, nh, inter, layers, dt))
            assert rc == 0, (H, dt)
            counts[H] = L.mb_bert_param_count(h)
            assert L.mb_bert_workspace_bytes(h) > 0
            L.mb_bert_destroy(h)
    assert counts[256] < counts[512] < counts[768] < counts[1024]
    assert 337e6 < counts[1024] < 338e6                           # bert-large 335.1 M + MAG 2.3 M + head, 64-float alignment included
    assert _create(_cfg(384, 6, 1536, 2))[0] == MB_ERR_SHAPE     # not one of the four
    assert _create(_cfg(1280, 20, 5120, 2))[0] == MB_ERR_SHAPE
    assert _create(_cfg(1024, 12, 4096, 2))[0] == MB_ERR_SHAPE   # heads of 64 only
    assert _create(_cfg(256, 8, 1024, 2))[0] == MB_ERR_SHAPE
    assert _create(_cfg(1024, 16, 4096, 0))[0] == MB_ERR_SHAPE   # at least one layer
    assert _create(_cfg(1024, 16, 4000, 2))[0] == MB_ERR_SHAPE   # intermediate_size % 128, as before
    for layers in (1, 5, 30, 40):                                 # any depth (above 30 the LayerNorm reductions go layer by layer)
        rc, h = _create(_cfg(256, 4, 1024, layers))
        assert rc == 0, layers
        L.mb_bert_destroy(h)


def test_large_parameter_table_is_the_oracles_state_dict():
    L = _lib.lib()
    H, nh, inter, layers = SIZES[0]
    rc, h = _create(_cfg(H, nh, inter, layers))
    assert rc == 0
    rows = _table(h)
    with torch.device("meta"):
        o = R.MAG_BertForSequenceClassification(R.BertConfigLite(**size_config(H)), R.MultimodalConfig(1.0, 0.5), 47, 74)
    want = {k: tuple(v.shape) for k, v in o.state_dict().items()}
    got = {r[0]: r[3] for r in rows}
    assert got == want
    # decay group first, then the no-decay group (the driver's split: "bias", "LayerNorm.*" do not decay); 64-float alignment; no overlap
    nd, n = L.mb_bert_decay_count(h), L.mb_bert_param_count(h)
    no_decay = ("bias", "LayerNorm.bias", "LayerNorm.weight")
    end = 0
    for name, off, numel, shape, dec in sorted(rows, key=lambda r: r[1]):
        assert off % 64 == 0 and off >= end and numel == int(np.prod(shape)), name
        end = off + numel
        assert dec == (0 if any(k in name for k in no_decay) else 1), name
        assert (off + numel <= nd) if dec else (off >= nd), name
    assert end <= n and nd % 64 == 0
    b, e = C.c_size_t(), C.c_size_t()
    L.mb_bert_shadow_range(h, C.byref(b), C.byref(e))
    per_layer = 4 * H * H + 2 * H * inter
    assert b.value == 0 and e.value == layers * per_layer + H * H          # every layer's GEMM weights + the pooler, contiguous
    L.mb_bert_destroy(h)


@pytest.mark.parametrize("H", [s[0] for s in SIZES])
def test_oracle_reproduces_the_reference_fixture(golden, H):
    g = golden["g11_bert_sizes"]
    o = {}
    for (B, L, V, seed) in CASES:
        if V not in o:
            m = R.MAG_BertForSequenceClassification(R.BertConfigLite(**size_config(H)), R.MultimodalConfig(1.0, 0.5), V, 74)
            o[V] = R.load_deterministic(m, "test").eval()
        b = weights.synthetic_bert_batch(B, L, V, 74, seed=seed)
        t = lambda k: torch.from_numpy(b[k])
        with torch.no_grad():
            logits = o[V](t("input_ids"), t("visual"), t("acoustic"), attention_mask=t("input_mask"), token_type_ids=t("segment_ids"))[0]
            seq = o[V].bert(t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"))[0]
        ref = g[key("logits", H, B, L, V, seed)]
        assert ref.shape == (B, 1)
        assert float(np.abs(logits.numpy() - ref).max()) <= 2e-5
        assert float(np.abs(weights.strided_sample(seq.numpy(), SAMPLE) - g[key("seq", H, B, L, V, seed)]).max()) <= 2e-5


def test_fixture_is_small_and_complete(golden):
    g = golden["g11_bert_sizes"]
    assert sorted(g.files) == sorted(key(k, s[0], *c) for k in ("logits", "seq") for s in SIZES for c in CASES)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g11_bert_sizes.npz")) < 16 * 1024


def test_config_size_check_names_the_supported_set():
    for kw in (dict(hidden_size=384, num_attention_heads=6, intermediate_size=1536),
               dict(hidden_size=1024, num_attention_heads=12, intermediate_size=4096)):
        with pytest.raises(ValueError) as ei:
            mb_bert.check_bert_sizes(BertConfig(**kw))
        assert "256, 512, 768, 1024" in str(ei.value)
        with pytest.raises(ValueError) as ei:          # the model constructor says the same, before it looks for a device
            MAG_BertForSequenceClassification(BertConfig(**kw), MultimodalConfig(1.0, 0.5))
        assert "256, 512, 768, 1024" in str(ei.value)
    with pytest.raises(ValueError):
        mb_bert.check_bert_sizes(BertConfig(intermediate_size=3000))
    for (H, nh, inter, layers) in SIZES:
        mb_bert.check_bert_sizes(BertConfig(**size_config(H)))
    mb_bert.check_bert_sizes(BertConfig())
    c = BertConfig.large(num_labels=3)
    assert (c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.intermediate_size, c.num_labels) == (1024, 16, 24, 4096, 3)
    assert "1024" in BertConfig.__doc__ and "bert-large" in BertConfig.__doc__


def test_config_json_beside_a_checkpoint_selects_the_model_size(tmp_path):
    """what from_pretrained does without config=: the directory's config.json (only the keys BertConfig knows) -> the engine's parameter
    table for that configuration takes the state dict saved from the oracle of the same size"""
    H, nh, inter, layers = SIZES[2]
    o = R.load_deterministic(R.MAG_BertForSequenceClassification(R.BertConfigLite(**size_config(H)), R.MultimodalConfig(1.0, 0.5), 47, 74), "test")
    torch.save(o.state_dict(), tmp_path / "pytorch_model.bin")
    hf = {"architectures": ["BertForMaskedLM"], "model_type": "bert", "transformers_version": "4.6.0", "gradient_checkpointing": False,
          "position_embedding_type": "absolute", "use_cache": True, "hidden_size": H, "num_attention_heads": nh, "intermediate_size": inter,
          "num_hidden_layers": layers, "vocab_size": 30522, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "max_position_embeddings": 512,
          "type_vocab_size": 2, "pad_token_id": 0, "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.1, "initializer_range": 0.02}
    (tmp_path / "config.json").write_text(json.dumps(hf))
    for where in (str(tmp_path), str(tmp_path / "pytorch_model.bin")):
        c = mb_bert.read_config_beside(where, num_labels=1)
        assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers, c.num_labels) == (H, nh, inter, layers, 1)
        assert not hasattr(c, "architectures") and not hasattr(c, "use_cache")
    assert MAG_BertForSequenceClassification._config_beside(str(tmp_path), 1).hidden_size == H
    rc, h = _create(_cfg(c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers))
    assert rc == 0
    got = {r[0]: r[3] for r in _table(h)}
    _lib.lib().mb_bert_destroy(h)
    sd = torch.load(tmp_path / "pytorch_model.bin", map_location="cpu")
    assert got == {k: tuple(v.shape) for k, v in sd.items()}
    # no json: bert-base stays the default
    os.remove(tmp_path / "config.json")
    assert mb_bert.read_config_beside(str(tmp_path)) is None
    assert MAG_BertForSequenceClassification._default_config(1).hidden_size == 768
    from bert_multimodal_transformer_amd.xlnet import MAG_XLNetForSequenceClassification
    (tmp_path / "config.json").write_text(json.dumps(hf))
    assert MAG_XLNetForSequenceClassification._config_beside(str(tmp_path), 1) is None          # MAG-BERT only


def test_driver_knows_bert_large():
    from bert_multimodal_transformer_amd import multimodal_driver as D
    a = D.parse_args(["--model", "bert-large-uncased", "--synthetic", "8"])
    assert a.model == "bert-large-uncased" and a.model in D.BERT_MODELS
    c = D.bert_config(a.model)
    assert (c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.intermediate_size) == (1024, 16, 24, 4096)
    assert D.bert_config("bert-base-uncased").hidden_size == 768
    with pytest.raises(SystemExit):
        D.parse_args(["--model", "bert-huge"])
    # the feature layout of a BERT model
    old = getattr(D, "args", None)
    try:
        D.args = a
        D.args.max_seq_length = 8
        tok = type("T", (), {"cls_token": "[CLS]", "sep_token": "[SEP]", "tokenize": lambda s, w: [w],
                             "convert_tokens_to_ids": lambda s, t: [7] * len(t)})()
        f = D.convert_to_features([((["a", "b"], np.ones((2, 47)), np.ones((2, 74))), 1.0, "s")], 8, tok)[0]
        assert f.input_mask == [1, 1, 1, 1, 0, 0, 0, 0] and f.segment_ids == [0] * 8
    finally:
        D.args = old


def test_step_bench_has_the_size_flags():
    src = open(os.path.join(ROOT, "tools", "step_bench.cpp")).read()
    for flag in ("--hidden", "--heads", "--inter", "--layers"):
        assert src.count('"%s"' % flag) >= 1, flag          # parsed
        assert ("[%s " % flag) in src, flag                   # in the usage comment
    assert "c.hidden_size = hidden" in src and "c.num_heads = heads" in src and "c.intermediate_size = inter" in src
    hdr = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    assert "1024" in hdr and "256" in hdr
