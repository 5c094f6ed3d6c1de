"""Writes tests/golden/g14_bert_injection.npz: eval logits and a strided sample of the final sequence output of MAG-BERT with the
Multimodal Adaptation Gate applied in front of encoder layer j instead of behind the embeddings, at 3 layers x 256 wide / 4 heads / inner
1024 with "test" weights and p_mag = 0.5, for j in INDICES on the batches CASES = (B, L, V): synthetic_bert_batch(seed=SEED).

The reference's MAG_BertModel.forward knows the gate behind the embeddings only, and so does the oracle's.  Run where the reference
checkout and transformers are available (the shim of oracle/make_golden.py), main() composes the REFERENCE's own module objects in
the moved order -- embeddings, encoder.layer[:j], MAG, encoder.layer[j:], pooler, dropout, classifier of its
MAG_BertForSequenceClassification -- asserts that composition == the oracle with patch_oracle(o, j) applied to 2e-5, and stores
results only: inputs and weights are regenerated from oracle/weights.py.  INDICES, CASES, SEED, SAMPLE, P_MAG, size_kw, key,
build_oracle and patch_oracle are what the tests import."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HEADS, INNER, LAYERS = 256, 4, 1024, 3
INDICES = (1, 2)
CASES = ((3, 20, 47), (4, 50, 35))         # B, L, V
A_DIM = 74
SEED = 11
SAMPLE = 64
P_MAG = 0.5


def size_kw(num_labels=1, **over):
    """keyword arguments of BertConfig / BertConfigLite for the fixture's model"""
    kw = dict(hidden_size=H, num_attention_heads=HEADS, intermediate_size=INNER, num_hidden_layers=LAYERS, num_labels=num_labels)
    kw.update(over)
    return kw


def key(kind, j, case):
    return "%s/j%d/B%d_L%d_V%d" % ((kind, j) + tuple(case))


def patch_oracle(o, j):
    """oracle.mag_bert_ref model `o` (MAG_BertForSequenceClassification or MAG_BertModel) with the gate in front of encoder layer j:
    the forward of its MAG_BertModel INSTANCE becomes embeddings -> layers [:j] -> MAG -> layers [j:] -> pooler.  Modules, parameters
    and dropout objects stay (replayed dropout masks keep working); j = 0 runs the same operations in the same order as the class's
    own forward.  The patched base model also keeps the tensor every layer read in `layer_inputs` (entry j is the gate's output,
    the last entry the sequence output) -- the hidden_states convention of the engine."""
    base = o.bert if hasattr(o, "bert") else o
    assert type(base).__name__ == "MAG_BertModel"
    NL = len(base.encoder.layer)
    if not 0 <= j < NL:
        raise ValueError("injection_index = %d outside [0, num_hidden_layers = %d)" % (j, NL))

    def forward(input_ids, visual, acoustic, attention_mask=None, token_type_ids=None, head_mask=None, inputs_embeds=None,
                position_ids=None):
        shape = input_ids.shape if input_ids is not None else inputs_embeds.shape[:-1]
        dev = visual.device
        if attention_mask is None:
            attention_mask = torch.ones(shape, dtype=torch.long, device=dev)
        if token_type_ids is None:
            token_type_ids = torch.zeros(shape, dtype=torch.long, device=dev)
        if head_mask is not None:
            head_mask = head_mask.to(torch.float32)
            if head_mask.dim() == 1:
                head_mask = head_mask[None].expand(NL, -1)
            head_mask = head_mask[:, None, :, None, None]
        ext = (1.0 - attention_mask[:, None, None, :].to(torch.float32)) * -10000.0
        x = base.embeddings(input_ids, token_type_ids, inputs_embeds, position_ids)
        reads = []
        for i, lyr in enumerate(base.encoder.layer):
            if i == j:
                x = base.MAG(x, visual, acoustic)
            reads.append(x)
            x = lyr(x, ext, None if head_mask is None else head_mask[i])
        base.layer_inputs = tuple(reads) + (x,)
        return x, base.pooler(x)

    base.forward = forward
    base.injection_index = j
    return o


def build_oracle(j, V, num_labels=1, p_mag=P_MAG, mode="test", **over):
    """the fixture's model as the oracle builds it, "test" weights, gate in front of layer j (None: the unpatched oracle)"""
    from oracle import mag_bert_ref as R
    o = R.MAG_BertForSequenceClassification(R.BertConfigLite(**size_kw(num_labels, **over)), R.MultimodalConfig(1.0, p_mag), V, A_DIM)
    R.load_deterministic(o, mode)
    return o if j is None else patch_oracle(o, j)


def main():
    from oracle.make_golden import GOLD, MC, _load, _maxdiff, _tb, install_shim
    from oracle import weights
    torch.manual_seed(0)
    cb, modeling, bert, _ = install_shim()
    out = {}
    for case in CASES:
        B, L, V = case
        modeling.TEXT_DIM = H
        modeling.VISUAL_DIM = bert.VISUAL_DIM = V
        try:
            cfg = cb.BertConfig(**size_kw())
            cfg._attn_implementation = "eager"
            ref = bert.MAG_BertForSequenceClassification(cfg, MC(1.0, P_MAG))
        finally:
            modeling.TEXT_DIM = 768
            modeling.VISUAL_DIM = bert.VISUAL_DIM = 47
        _load(ref, "test")
        ref.eval()
        ids, vis, aco, mask, seg, lab = _tb(weights.synthetic_bert_batch(B, L, V, A_DIM, seed=SEED))
        rb = ref.bert
        for j in INDICES:
            mine = build_oracle(j, V)
            mine.eval()
            with torch.no_grad():
                # the reference's own modules, composed in the moved order
                ext = rb.get_extended_attention_mask(mask, ids.shape, ids.device)
                x = rb.embeddings(input_ids=ids, position_ids=None, token_type_ids=seg, inputs_embeds=None)
                for i, lyr in enumerate(rb.encoder.layer):
                    if i == j:
                        x = rb.MAG(x, vis, aco)
                    y = lyr(x, attention_mask=ext)
                    x = y[0] if isinstance(y, (tuple, list)) else y
                sa = x
                a = ref.classifier(ref.dropout(rb.pooler(sa)))
                b = mine(ids, vis, aco, attention_mask=mask, token_type_ids=seg)[0]
                sb = mine.bert(ids, vis, aco, mask, seg)[0]
            d, ds = _maxdiff(a, b), _maxdiff(sa, sb)
            print("G14 MAG-BERT j=%d %s reference modules vs patched oracle max |diff| logits %.3g, sequence_output %.3g; logits %s"
                  % (j, case, d, ds, a.view(-1).tolist()))
            assert tuple(sa.shape) == (B, L, H) and d < 2e-5 and ds < 2e-5
            out[key("logits", j, case)] = a.numpy()
            out[key("seq", j, case)] = weights.strided_sample(sa.numpy(), SAMPLE)
    np.savez(os.path.join(GOLD, "g14_bert_injection.npz"), **out)


if __name__ == "__main__":
    main()
