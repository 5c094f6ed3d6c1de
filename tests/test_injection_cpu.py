"""CPU: MAG-BERT with the gate in front of any encoder layer (mb_bert_config.injection_index) -- the engine's argument check, the parameter
layout that must not depend on the index, the one workspace tensor it costs, the Python constructors' ValueError, patch_oracle of
scripts/make_golden_injection.py against tests/golden/g14_bert_injection.npz, and the driver's flag.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from bert_multimodal_transformer_amd import BertConfig, MAG_BertForSequenceClassification, MAG_BertModel, MultimodalConfig, _lib
from bert_multimodal_transformer_amd import bert as mb_bert
from oracle import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_injection import A_DIM, CASES, INDICES, LAYERS, SAMPLE, SEED, build_oracle, key, patch_oracle, size_kw      # noqa: E402

MB_ERR_ARG = 1004
NL = 4


def _cfg_args(H=256, layers=NL, dtype=_lib.DT_BF16, max_batch=3, max_seq=50):
    """the twenty values in front of hidden_act"""
    return (30522, H, layers, H // 64, 4 * H, 512, 2, 1, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, dtype, max_batch, max_seq)


def _cfg(inj=None, H=256, layers=NL, dtype=_lib.DT_BF16, max_batch=3, max_seq=50):
    """inj = None: a config built without the field (it stays zero, like a C caller's `= {}`)"""
    args = _cfg_args(H, layers, dtype, max_batch, max_seq) + (0,)
    return _lib.BertEngineConfig(*(args if inj is None else args + (inj,)))


def _create(cfg):
    h = C.c_void_p()
    return _lib.lib().mb_bert_create(C.byref(cfg), C.byref(h)), h


def _layout(h):
    L = _lib.lib()
    rows = []
    for i in range(L.mb_bert_num_tensors(h)):
        name = C.create_string_buffer(160)
        off, numel, ndim, dec = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
        shp = (C.c_int64 * 4)()
        assert L.mb_bert_tensor_info(h, i, name, 160, C.byref(off), C.byref(numel), C.byref(ndim), shp, C.byref(dec)) == 0
        rows.append((name.value.decode(), off.value, numel.value, tuple(shp[k] for k in range(ndim.value)), dec.value))
    b, e = C.c_size_t(), C.c_size_t()
    L.mb_bert_shadow_range(h, C.byref(b), C.byref(e))
    return rows, L.mb_bert_param_count(h), L.mb_bert_decay_count(h), (b.value, e.value)


def test_config_field_mirrors_the_header_and_defaults_to_zero():
    """hidden_act stays the last field of mb_bert_config (tests/test_activations_cpu.py pins it), so the new field lies in front of it, in
    the header and in the ctypes mirror alike; positional arguments keep the order in which the fields were added"""
    names = [f[0] for f in _lib.BertEngineConfig._fields_]
    assert names[-2:] == ["injection_index", "hidden_act"]
    assert _lib.BertEngineConfig.POSITIONAL[-2:] == ("hidden_act", "injection_index") and sorted(_lib.BertEngineConfig.POSITIONAL) == sorted(names)
    c = _cfg()
    assert c.injection_index == 0 and _cfg(2).injection_index == 2
    c = _lib.BertEngineConfig(*([7] * 20), 3, 2)
    assert (c.max_seq, c.hidden_act, c.injection_index) == (7, 3, 2)
    assert _lib.BertEngineConfig(*([7] * 20), 3).injection_index == 0 and _lib.BertEngineConfig(injection_index=5, hidden_act=1).injection_index == 5
    for bad in (lambda: _lib.BertEngineConfig(*([0] * 23)), lambda: _lib.BertEngineConfig(no_such_field=1)):
        with pytest.raises(TypeError):
            bad()
    hdr = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    body = hdr[hdr.index("typedef struct {", hdr.index("MAG-BERT engine")):hdr.index("} mb_bert_config;")]
    # the header's fields in order, comments taken off: the same names in the same order as the ctypes mirror
    import re
    decl = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for stmt in decl.split(";") for n in re.sub(r"^\s*(typedef struct \{)?\s*(int|float)\s", "", stmt.strip()).split(",") if n.strip()]
    assert fields == names, (fields, names)
    # the engine reads the field where the mirror writes it: a one-layer engine takes index 0 and refuses 1, whatever hidden_act says
    for act in (0, 4):
        assert _create(_lib.BertEngineConfig(*_cfg_args(layers=1), act, 1))[0] == MB_ERR_ARG
        rc, h = _create(_lib.BertEngineConfig(*_cfg_args(layers=1), act, 0))
        assert rc == 0
        _lib.lib().mb_bert_destroy(h)


def test_create_refuses_an_index_without_a_layer():
    for inj in (-1, NL, NL + 3):
        rc, _ = _create(_cfg(inj))
        assert rc == MB_ERR_ARG, inj
    for inj in (0, 1, NL - 1):
        rc, h = _create(_cfg(inj))
        assert rc == 0, inj
        _lib.lib().mb_bert_destroy(h)
    rc, _ = _create(_cfg(1, layers=1))
    assert rc == MB_ERR_ARG


def test_parameter_layout_does_not_depend_on_the_index():
    got = []
    for inj in (0, 1, NL - 1):
        rc, h = _create(_cfg(inj))
        assert rc == 0
        got.append(_layout(h))
        _lib.lib().mb_bert_destroy(h)
    assert got[0] == got[1] == got[2]
    assert any(r[0] == "bert.MAG.W_hv.weight" for r in got[0][0])


@pytest.mark.parametrize("dtype,esize", [(_lib.DT_BF16, 2), (_lib.DT_F32, 4)])
def test_workspace_grows_by_exactly_the_pre_gate_tensor(dtype, esize):
    L = _lib.lib()

    def ws(inj, H, B, S):
        rc, h = _create(_cfg(inj, H=H, dtype=dtype, max_batch=B, max_seq=S))
        assert rc == 0
        n = L.mb_bert_workspace_bytes(h)
        L.mb_bert_destroy(h)
        return n

    for (H, B, S) in ((256, 3, 50), (768, 4, 50), (256, 2, 200)):       # T = 150, 200 (both padded to the next 64) and 400 (tiled attention)
        base = ws(None, H, B, S)
        assert ws(0, H, B, S) == base
        rows = (B * S + 63) // 64 * 64
        for inj in (1, NL - 1):
            assert ws(inj, H, B, S) - base == rows * H * esize, (H, B, S, inj)


def test_constructors_name_the_index_and_the_depth_before_any_device():
    for inj in (3, 7, -1):
        for cls in (MAG_BertForSequenceClassification, MAG_BertModel):
            with pytest.raises(ValueError) as ei:
                cls(BertConfig(num_hidden_layers=3), MultimodalConfig(1.0, 0.5), injection_index=inj)
            assert "injection_index" in str(ei.value) and "num_hidden_layers" in str(ei.value)
            assert str(inj) in str(ei.value) and "3" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        MAG_BertForSequenceClassification.from_pretrained("/nonexistent", MultimodalConfig(1.0, 0.5), config=BertConfig(num_hidden_layers=2),
                                                          injection_index=2)
    assert "injection_index" in str(ei.value)
    mb_bert.check_bert_sizes(BertConfig(num_hidden_layers=3), 2)
    mb_bert.check_bert_sizes(BertConfig(num_hidden_layers=1), 0)
    mb_bert.check_bert_sizes(BertConfig())                                # the size check alone, as before
    with pytest.raises(ValueError):
        mb_bert.check_bert_sizes(BertConfig(num_hidden_layers=3), 3)


def _batch(case):
    B, L, V = case
    b = weights.synthetic_bert_batch(B, L, V, A_DIM, seed=SEED)
    return tuple(torch.from_numpy(b[k]) for k in ("input_ids", "visual", "acoustic", "input_mask", "segment_ids"))


@pytest.mark.parametrize("j", INDICES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_L%d_V%d" % c)
def test_patched_oracle_reproduces_the_fixture(golden, j, case):
    g = golden["g14_bert_injection"]
    o = build_oracle(j, case[2]).eval()
    ids, vis, aco, mask, seg = _batch(case)
    with torch.no_grad():
        logits = o(ids, vis, aco, attention_mask=mask, token_type_ids=seg)[0]
        seq = o.bert(ids, vis, aco, mask, seg)[0]
    assert g[key("logits", j, case)].shape == (case[0], 1)
    assert float(np.abs(logits.numpy() - g[key("logits", j, case)]).max()) <= 2e-5
    assert float(np.abs(weights.strided_sample(seq.numpy(), SAMPLE) - g[key("seq", j, case)]).max()) <= 2e-5
    # the tensors the layers read: entry j is the gate's output, and the position of the gate matters to the result
    reads = o.bert.layer_inputs
    assert len(reads) == LAYERS + 1 and torch.equal(reads[-1], seq)
    other = build_oracle(3 - j, case[2]).eval()
    with torch.no_grad():
        assert float((other(ids, vis, aco, attention_mask=mask, token_type_ids=seg)[0] - logits).abs().max()) > 1e-4


def test_fixture_is_small_and_complete(golden):
    g = golden["g14_bert_injection"]
    assert sorted(g.files) == sorted(key(k, j, c) for k in ("logits", "seq") for j in INDICES for c in CASES)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_bert_injection.npz")) < 16 * 1024


def test_patch_at_zero_is_the_unpatched_oracle_bit_for_bit():
    case = CASES[0]
    plain, zero = build_oracle(None, case[2]), build_oracle(0, case[2])
    ids, vis, aco, mask, seg = _batch(case)
    for train in (False, True):                     # train: the same dropout draws in the same order
        outs = []
        for m in (plain, zero):
            m.train(train)
            torch.manual_seed(5)
            with torch.no_grad():
                outs.append((m(ids, vis, aco, attention_mask=mask, token_type_ids=seg)[0],) + tuple(m.bert(ids, vis, aco, mask, seg)))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    with pytest.raises(ValueError):
        patch_oracle(build_oracle(None, case[2]), LAYERS)
    # a patched model keeps its modules and parameters: same state dict
    assert list(plain.state_dict()) == list(zero.state_dict())
    assert size_kw()["num_hidden_layers"] == LAYERS


def test_driver_takes_the_flag_and_keeps_each_models_default():
    from bert_multimodal_transformer_amd import multimodal_driver as D
    from bert_multimodal_transformer_amd.global_configs import XLNET_INJECTION_INDEX
    a = D.parse_args(["--synthetic", "8"])
    assert a.injection_index is None and D.injection_index_of(a) == 0
    a = D.parse_args(["--synthetic", "8", "--model", "bert-large-uncased"])
    assert D.injection_index_of(a) == 0
    for m in D.XLNET_MODELS:
        assert D.injection_index_of(D.parse_args(["--synthetic", "8", "--model", m])) == XLNET_INJECTION_INDEX
    a = D.parse_args(["--synthetic", "8", "--injection_index", "6"])
    assert a.injection_index == 6 and D.injection_index_of(a) == 6
    a = D.parse_args(["--synthetic", "8", "--model", "xlnet-base-cased", "--injection_index", "0"])
    assert D.injection_index_of(a) == 0
    with pytest.raises(SystemExit):
        D.parse_args(["--injection_index", "first"])


def test_step_bench_takes_the_flag_for_both_models():
    src = open(os.path.join(ROOT, "tools", "step_bench.cpp")).read()
    assert '"--inject"' in src and "c.injection_index = " in src and "xc.injection_index = inject" in src
