"""Writes tests/golden/g10_xlnet_long.npz: eval logits of the REFERENCE's own MAG_XLNetForSequenceClassification (12 layers, "test"
weights) on sequences longer than 128 rows -- (B=2, L=256, seed 51) and (B=2, L=512, seed 53).  Run where the reference checkout and
transformers are available (the shim of oracle/make_golden.py); asserts reference == oracle to 2e-5 like gen_xlnet and stores the
logits only: inputs and weights are regenerated from oracle/weights.py (long_batch below, which the tests import)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((2, 256, 51), (2, 512, 53))


def long_batch(B, L, seed, V=47, A=74, short=5):
    """synthetic_xlnet_batch with row 0 at full length (keys beyond 128 live) and row 1 at `short` tokens (min_len = 5; left padding: the
    first key tiles of that row are all padding).  The tests import this function: one construction for the fixture and its readers."""
    from oracle import weights
    b = weights.synthetic_xlnet_batch(B, L, V, A, seed=seed)
    for r, k in ((0, L - 2), (1, short)):
        if r >= B:
            continue
        pad = L - k - 2
        b["input_ids"][r] = 5
        b["input_ids"][r, pad:pad + k] = 10 + (np.arange(k) * 7919) % 31990
        b["input_ids"][r, L - 2] = 4
        b["input_ids"][r, L - 1] = 3
        b["input_mask"][r] = 0
        b["input_mask"][r, pad:] = 1
        b["segment_ids"][r] = 3
        b["segment_ids"][r, pad:L - 1] = 0
        b["segment_ids"][r, L - 1] = 2
        b["visual"][r] = weights.uniform("xlong%d.vis%d" % (seed, r), (L, V), -2.0, 2.0)
        b["acoustic"][r] = weights.uniform("xlong%d.aco%d" % (seed, r), (L, A), -2.0, 2.0)
        for key in ("visual", "acoustic"):
            b[key][r, :pad] = 0
            b[key][r, L - 2:] = 0
    return b


def main():
    from oracle.make_golden import GOLD, MC, _load, _tb, install_shim
    from oracle import mag_xlnet_ref as X
    torch.manual_seed(0)
    cb, modeling, bert, xlnet = install_shim()
    from transformers.models.xlnet import configuration_xlnet as cx
    modeling.VISUAL_DIM = 47
    cfg = cx.XLNetConfig(d_model=768, n_layer=12, n_head=12, d_inner=3072, mem_len=None, num_labels=1)
    ref = xlnet.MAG_XLNetForSequenceClassification(cfg, MC(1.0, 0.5))
    _load(ref, "test")
    mine = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(n_layer=12), X.MultimodalConfig(1.0, 0.5), 47, 74)
    mine.load_state_dict(ref.state_dict(), strict=True)
    ref.eval(); mine.eval()
    out = {}
    for (B, L, seed) in CASES:
        ids, vis, aco, mask, seg, lab = _tb(long_batch(B, L, seed))
        with torch.no_grad():
            a = ref(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None)[0]
            b = mine(ids, vis, aco, mask, seg)[0]
        d = float((a - b).abs().max())
        print("G10 xlnet long B=%d L=%d seed=%d: reference vs oracle max |diff| = %.3g, logits %s" % (B, L, seed, d, a.view(-1).tolist()))
        assert d < 2e-5
        out["logits/B%d_L%d_seed%d" % (B, L, seed)] = a.numpy()
    np.savez(os.path.join(GOLD, "g10_xlnet_long.npz"), **out)


if __name__ == "__main__":
    main()
