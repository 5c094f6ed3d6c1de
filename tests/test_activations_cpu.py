"""CPU: the feed-forward activations next to erf-GELU -- configuration names, the driver's --hidden_act, the engine-config structs, and
the references the GPU tests lean on: tests/golden/g13_activations.npz (the reference's own models, scripts/make_golden_activations.py)
against the CPU oracle with the activation patched in, and what separates the five activations at model level."""
import ctypes as C
import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from bert_multimodal_transformer_amd import BertConfig, XLNetConfig, _lib
from oracle import mag_bert_ref as R, mag_xlnet_ref as X, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_activations import ACTS, CASE, SAMPLE, SEEDS, act_fn, key, patch_oracle, size_kw      # noqa: E402


def test_config_names():
    for name in ACTS + ("silu",):
        assert BertConfig(hidden_act=name).hidden_act == name
        assert XLNetConfig(ff_activation=name).ff_activation == name
    assert [_lib.activation_code(n, "hidden_act") for n in ACTS] == [0, 1, 2, 3, 4]
    assert _lib.activation_code("silu", "hidden_act") == _lib.ACT_SWISH
    assert (_lib.EPI_BIAS_RELU, _lib.EPI_BIAS_SWISH, _lib.EPI_BIAS_GELU_NEW, _lib.EPI_BIAS_MISH) == (7, 8, 9, 10)
    for bad in ("tanh", "gelu_fast", "GELU", "", None, torch.nn.functional.relu):
        with pytest.raises(NotImplementedError) as ex:
            BertConfig(hidden_act=bad)
        assert all(n in str(ex.value) for n in ACTS)                      # the message names what is built
        with pytest.raises(NotImplementedError):
            XLNetConfig(ff_activation=bad)
    with pytest.raises(NotImplementedError):                                # XLNet's other refusals stay
        XLNetConfig(ff_activation="relu", attn_type="uni")
    with pytest.raises(NotImplementedError):
        XLNetConfig(summary_type="mean")


def test_from_json_file_reads_the_activation(tmp_path):
    (tmp_path / "b.json").write_text(json.dumps(dict(size_kw("bert"), hidden_act="gelu_new", model_type="bert")))
    (tmp_path / "x.json").write_text(json.dumps(dict(size_kw("xlnet"), ff_activation="silu", model_type="xlnet")))
    (tmp_path / "bad.json").write_text(json.dumps(dict(size_kw("bert"), hidden_act="tanh")))
    assert BertConfig.from_json_file(str(tmp_path / "b.json")).hidden_act == "gelu_new"
    assert XLNetConfig.from_json_file(str(tmp_path / "x.json")).ff_activation == "silu"
    with pytest.raises(NotImplementedError):
        BertConfig.from_json_file(str(tmp_path / "bad.json"))


def test_driver_option():
    from bert_multimodal_transformer_amd import multimodal_driver as D
    assert D.parse_args([]).hidden_act is None
    assert D.parse_args(["--hidden_act", "mish"]).hidden_act == "mish"
    with pytest.raises(SystemExit):
        D.parse_args(["--hidden_act", "tanh"])
    assert D.with_hidden_act(D.bert_config("bert-base-uncased"), "relu").hidden_act == "relu"
    assert D.with_hidden_act(D.xlnet_config("xlnet-base-cased"), "swish").ff_activation == "swish"
    assert D.with_hidden_act(D.bert_config("bert-base-uncased"), None).hidden_act == "gelu"


def _bert_cfg(act):
    return _lib.BertEngineConfig(30522, 256, 2, 4, 1024, 512, 2, 1, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_F32, 4, 50, act)


def _xlnet_cfg(act):
    return _lib.XlnetEngineConfig(32000, 256, 2, 4, 1024, 1, 47, 74, 1, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_F32, 4, 50, act)


def test_engine_config_structs(tmp_path):
    """the appended field: positional construction with the old 20 / 18 values leaves it 0 (gelu); it round-trips through create (codes
    0 .. 4 make an engine, anything else is MB_ERR_ARG); and, where a C compiler is at hand, sizeof agrees with the header"""
    assert _lib.BertEngineConfig(*([0] * 20)).hidden_act == 0 and _lib.XlnetEngineConfig(*([0] * 18)).ff_activation == 0
    assert _lib.BertEngineConfig._fields_[-1][0] == "hidden_act" and _lib.XlnetEngineConfig._fields_[-1][0] == "ff_activation"
    L = _lib.lib()
    for cfg_of, create, destroy in ((_bert_cfg, L.mb_bert_create, L.mb_bert_destroy), (_xlnet_cfg, L.mb_xlnet_create, L.mb_xlnet_destroy)):
        for act in range(5):
            h = C.c_void_p()
            cfg = cfg_of(act)
            _lib.check(create(C.byref(cfg), C.byref(h)))
            destroy(h)
        for bad in (5, -1, 7):
            h = C.c_void_p()
            cfg = cfg_of(bad)
            assert create(C.byref(cfg), C.byref(h)) == 1004 and not h.value
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        src = tmp_path / "s.c"
        src.write_text('#include <stdio.h>\n#include "magbert_hip.h"\n'
                       'int main(void) { printf("%zu %zu\\n", sizeof(mb_bert_config), sizeof(mb_xlnet_config)); return 0; }\n')
        exe = tmp_path / "s"
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
        sizes = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(s) for s in sizes] == [C.sizeof(_lib.BertEngineConfig), C.sizeof(_lib.XlnetEngineConfig)], sizes


# ------------------------------------------------------------------------------------------------ the references
def _tb(b):
    t = lambda k: torch.from_numpy(b[k])
    return t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids")


@pytest.mark.parametrize("act", ACTS)
def test_patched_oracle_reproduces_the_reference_fixture(golden, act):
    g = golden["g13_activations"]
    B, L, V = CASE
    o = R.MAG_BertForSequenceClassification(R.BertConfigLite(**size_kw("bert")), R.MultimodalConfig(1.0, 0.5), V, 74)
    o = patch_oracle(R.load_deterministic(o, "test"), act).eval()
    c = _tb(weights.synthetic_bert_batch(B, L, V, 74, seed=SEEDS["bert"]))
    with torch.no_grad():
        logits = o(*c)[0]
        seq = o.bert(*c)[0]
    assert float(np.abs(logits.numpy() - g[key("bert", "logits", act)]).max()) <= 2e-5
    assert float(np.abs(weights.strided_sample(seq.numpy(), SAMPLE) - g[key("bert", "seq", act)]).max()) <= 2e-5
    x = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**size_kw("xlnet")), X.MultimodalConfig(1.0, 0.5), V, 74)
    x = patch_oracle(X.load_deterministic(x, "test"), act).eval()
    c = _tb(weights.synthetic_xlnet_batch(B, L, V, 74, seed=SEEDS["xlnet"]))
    with torch.no_grad():
        logits = x(*c)[0]
        seq = x.transformer(*c)
    assert float(np.abs(logits.numpy() - g[key("xlnet", "logits", act)]).max()) <= 2e-5
    assert float(np.abs(weights.strided_sample(seq.numpy(), SAMPLE) - g[key("xlnet", "seq", act)]).max()) <= 2e-5


def test_what_separates_the_activations(golden):
    """model level (the fixture): gelu / relu / swish / mish are pairwise > 10 x 1e-3 apart in the sequence-output sample -- the quantity
    tests/test_activations_model_gpu.py uses -- while their logits and gelu_new vs gelu are not; operator level (fp64): any two of the
    five differ in act' by more than 10 x the fp32 tolerance of test_ops_gpu.close() on [-6, 6]"""
    g = golden["g13_activations"]
    assert len(g.files) == 20 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "g13_activations.npz")) < 16 * 1024
    for model in ("bert", "xlnet"):
        for a, b in itertools.combinations(("gelu", "relu", "swish", "mish"), 2):
            assert float(np.abs(g[key(model, "seq", a)] - g[key(model, "seq", b)]).max()) > 10 * 1e-3, (model, a, b)
        assert float(np.abs(g[key(model, "seq", "gelu")] - g[key(model, "seq", "gelu_new")]).max()) < 1e-3
    u = torch.linspace(-6.0, 6.0, 4801, dtype=torch.float64)
    d = {}
    for a in ACTS:
        x = u.clone().requires_grad_(True)
        (d[a],) = torch.autograd.grad(act_fn(a)(x).sum(), x)
    for a, b in itertools.combinations(ACTS, 2):
        t = 2e-5 * max(float(d[a].abs().max()), float(d[b].abs().max())) + 1e-6
        assert float((d[a] - d[b]).abs().max()) > 10 * t, (a, b)
