"""Writes tests/golden/g11_bert_sizes.npz: eval logits and a strided sample of the sequence output of the REFERENCE's own
MAG_BertForSequenceClassification at the model sizes next to bert-base, at full depth and with "test" weights -- 24 x 1024 / 16 heads /
4096 (bert-large-uncased), 8 x 512 / 8 / 2048, 4 x 256 / 4 / 1024 -- on the batches (B=4, L=50, V=47, seed 11) and (B=3, L=128, V=35,
seed 13).  Run where the reference checkout and transformers are available (the shim of oracle/make_golden.py; the reference's MAG
takes its width from modeling.TEXT_DIM, set around each build like VISUAL_DIM); asserts reference == oracle to 2e-5 and stores results
only: inputs and weights are regenerated from oracle/weights.py.  SIZES, CASES, size_config and key are what the tests import."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (hidden_size, num_attention_heads, intermediate_size, num_hidden_layers)
SIZES = ((1024, 16, 4096, 24), (512, 8, 2048, 8), (256, 4, 1024, 4))
# (B, L, V, seed)
CASES = ((4, 50, 47, 11), (3, 128, 35, 13))
SAMPLE = 64


def size_config(H, layers=None, num_labels=1):
    """keyword arguments of BertConfig / BertConfigLite for hidden size H (layers: None = the full depth of SIZES)"""
    for (h, nh, inter, nl) in SIZES:
        if h == H:
            return dict(hidden_size=h, num_attention_heads=nh, intermediate_size=inter, num_hidden_layers=nl if layers is None else layers,
                        num_labels=num_labels)
    raise KeyError(H)


def key(kind, H, B, L, V, seed):
    return "%s/H%d/B%d_L%d_V%d_seed%d" % (kind, H, B, L, V, seed)


def main():
    from oracle.make_golden import GOLD, MC, _load, _tb, install_shim
    from oracle import mag_bert_ref as R
    from oracle import weights
    torch.manual_seed(0)
    cb, modeling, bert, xlnet = install_shim()
    out = {}
    for (H, nh, inter, nl) in SIZES:
        for (B, L, V, seed) in CASES:
            modeling.VISUAL_DIM = V
            bert.VISUAL_DIM = V
            modeling.TEXT_DIM = H
            try:
                cfg = cb.BertConfig(**size_config(H))
                cfg._attn_implementation = "eager"
                ref = bert.MAG_BertForSequenceClassification(cfg, MC(1.0, 0.5))
            finally:
                modeling.VISUAL_DIM = 47
                bert.VISUAL_DIM = 47
                modeling.TEXT_DIM = 768
            _load(ref, "test")
            mine = R.MAG_BertForSequenceClassification(R.BertConfigLite(**size_config(H)), R.MultimodalConfig(1.0, 0.5), V, 74)
            sd = {k: v for k, v in ref.state_dict().items() if "position_ids" not in k and "token_type_ids" not in k}
            mine.load_state_dict(sd, strict=True)
            ref.eval(); mine.eval()
            ids, vis, aco, mask, seg, lab = _tb(weights.synthetic_bert_batch(B, L, V, 74, seed=seed))
            with torch.no_grad():
                a = ref(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None)[0]
                sa = ref.bert(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0]
                b = mine(ids, vis, aco, attention_mask=mask, token_type_ids=seg)[0]
                sb = mine.bert(ids, vis, aco, mask, seg)[0]
            d, ds = float((a - b).abs().max()), float((sa - sb).abs().max())
            print("G11 %d x %d/%d/%d B=%d L=%d V=%d seed=%d: reference vs oracle max |diff| logits %.3g, sequence_output %.3g; logits %s"
                  % (nl, H, nh, inter, B, L, V, seed, d, ds, a.view(-1).tolist()))
            assert d < 2e-5 and ds < 2e-5
            out[key("logits", H, B, L, V, seed)] = a.numpy()
            out[key("seq", H, B, L, V, seed)] = weights.strided_sample(sa.numpy(), SAMPLE)
    np.savez(os.path.join(GOLD, "g11_bert_sizes.npz"), **out)


if __name__ == "__main__":
    main()
