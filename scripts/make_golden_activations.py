"""Writes tests/golden/g13_activations.npz: eval logits and a strided sample of the final sequence output of the REFERENCE's own
MAG_BertForSequenceClassification (config.hidden_act) and MAG_XLNetForSequenceClassification (config.ff_activation) for each of the
five feed-forward activations transformers 3.0.2 names -- gelu, relu, swish, gelu_new, mish -- at 2 layers x 256 wide / 4 heads / inner
1024 with "test" weights, on the batches (B=3, L=20, V=47): synthetic_bert_batch(seed=11) and synthetic_xlnet_batch(seed=31).  Run where
the reference checkout and transformers are available (the shim of oracle/make_golden.py); asserts reference == oracle with the activation
swapped in (patch_oracle below: the oracle's own text knows erf-GELU only) to 2e-5 and stores results only: inputs and weights are
regenerated from oracle/weights.py.  ACTS, CASE, SEEDS, SAMPLE, size_kw, key, act_fn and patch_oracle are what the tests import."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACTS = ("gelu", "relu", "swish", "gelu_new", "mish")
H, HEADS, INNER, LAYERS = 256, 4, 1024, 2
CASE = (3, 20, 47)                         # B, L, V
SEEDS = {"bert": 11, "xlnet": 31}
SAMPLE = 64


def size_kw(model, num_labels=1):
    """keyword arguments of BertConfig / BertConfigLite (model = "bert") or XLNetConfig / XLNetConfigLite ("xlnet")"""
    if model == "bert":
        return dict(hidden_size=H, num_attention_heads=HEADS, intermediate_size=INNER, num_hidden_layers=LAYERS, num_labels=num_labels)
    return dict(d_model=H, n_head=HEADS, d_inner=INNER, n_layer=LAYERS, num_labels=num_labels)


def key(model, kind, act):
    return "%s/%s/%s" % (model, kind, act)


def act_fn(name):
    """the activation as transformers 3.0.2 ACT2FN computes it (any floating dtype; autograd gives the derivative)"""
    F = torch.nn.functional
    if name == "gelu":
        return F.gelu
    if name == "relu":
        return F.relu
    if name in ("swish", "silu"):
        return lambda x: x * torch.sigmoid(x)
    if name == "gelu_new":
        return lambda x: 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))
    if name == "mish":
        return lambda x: x * torch.tanh(F.softplus(x))
    raise KeyError(name)


def patch_oracle(o, name):
    """oracle.mag_bert_ref / oracle.mag_xlnet_ref model `o` with activation `name` in its feed-forward blocks: the forward of every
    BertIntermediate / XLNetFeedForward INSTANCE is replaced (the modules, their parameters and their dropout objects stay)"""
    f = act_fn(name)
    n = 0
    for mod in o.modules():
        kind = type(mod).__name__
        if kind == "BertIntermediate":
            mod.forward = (lambda x, mod=mod: f(mod.dense(x)))
            n += 1
        elif kind == "XLNetFeedForward":
            def ff(inp, mod=mod):
                out = mod.dropout(f(mod.layer_1(inp)))
                out = mod.dropout(mod.layer_2(out))
                return mod.layer_norm(out + inp)
            mod.forward = ff
            n += 1
    assert n > 0, "no feed-forward block found"
    return o


def main():
    from transformers.models.xlnet import configuration_xlnet as cx
    from oracle.make_golden import GOLD, MC, _load, _maxdiff, _tb, install_shim
    from oracle import mag_bert_ref as R
    from oracle import mag_xlnet_ref as X
    from oracle import weights
    torch.manual_seed(0)
    cb, modeling, bert, xlnet = install_shim()
    B, L, V = CASE
    out = {}
    for act in ACTS:
        modeling.TEXT_DIM = H
        try:
            cfg = cb.BertConfig(hidden_act=act, **size_kw("bert"))
            cfg._attn_implementation = "eager"
            ref = bert.MAG_BertForSequenceClassification(cfg, MC(1.0, 0.5))
            xref = xlnet.MAG_XLNetForSequenceClassification(cx.XLNetConfig(mem_len=None, ff_activation=act, **size_kw("xlnet")), MC(1.0, 0.5))
        finally:
            modeling.TEXT_DIM = 768
        # MAG-BERT
        _load(ref, "test")
        mine = R.MAG_BertForSequenceClassification(R.BertConfigLite(**size_kw("bert")), R.MultimodalConfig(1.0, 0.5), V, 74)
        mine.load_state_dict({k: v for k, v in ref.state_dict().items() if "position_ids" not in k and "token_type_ids" not in k}, strict=True)
        patch_oracle(mine, act)
        ref.eval(); mine.eval()
        ids, vis, aco, mask, seg, lab = _tb(weights.synthetic_bert_batch(B, L, V, 74, seed=SEEDS["bert"]))
        with torch.no_grad():
            a = ref(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None)[0]
            sa = ref.bert(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0]
            b = mine(ids, vis, aco, attention_mask=mask, token_type_ids=seg)[0]
            sb = mine.bert(ids, vis, aco, mask, seg)[0]
        d, ds = _maxdiff(a, b), _maxdiff(sa, sb)
        print("G13 MAG-BERT  %-8s reference vs patched oracle max |diff| logits %.3g, sequence_output %.3g; logits %s" % (act, d, ds, a.view(-1).tolist()))
        assert tuple(sa.shape) == (B, L, H) and d < 2e-5 and ds < 2e-5
        out[key("bert", "logits", act)] = a.numpy()
        out[key("bert", "seq", act)] = weights.strided_sample(sa.numpy(), SAMPLE)
        # MAG-XLNet
        _load(xref, "test")
        xmine = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**size_kw("xlnet")), X.MultimodalConfig(1.0, 0.5), V, 74)
        xmine.load_state_dict(xref.state_dict(), strict=True)
        patch_oracle(xmine, act)
        xref.eval(); xmine.eval()
        ids, vis, aco, mask, seg, lab = _tb(weights.synthetic_xlnet_batch(B, L, V, 74, seed=SEEDS["xlnet"]))
        with torch.no_grad():
            a = xref(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None)[0]
            sa = xref.transformer(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0]
            b = xmine(ids, vis, aco, mask, seg)[0]
            sb = xmine.transformer(ids, vis, aco, mask, seg)
        d, ds = _maxdiff(a, b), _maxdiff(sa, sb)
        print("G13 MAG-XLNet %-8s reference vs patched oracle max |diff| logits %.3g, transformer output %.3g; logits %s" % (act, d, ds, a.view(-1).tolist()))
        assert tuple(sa.shape) == (B, L, H) and d < 2e-5 and ds < 2e-5
        out[key("xlnet", "logits", act)] = a.numpy()
        out[key("xlnet", "seq", act)] = weights.strided_sample(sa.numpy(), SAMPLE)
    np.savez(os.path.join(GOLD, "g13_activations.npz"), **out)


if __name__ == "__main__":
    main()
