"""Writes tests/golden/g12_xlnet_sizes.npz: eval logits and a strided sample of the transformer output of the REFERENCE's own
MAG_XLNetForSequenceClassification at the model sizes next to xlnet-base, at full depth and with "test" weights -- 24 x 1024 / 16 heads /
4096 (xlnet-large-cased), 8 x 512 / 8 / 2048, 4 x 256 / 4 / 1024 -- on the batches (B=4, L=50, V=47, seed 11) and (B=3, L=128, V=35,
seed 13); and, at 1024 with 2 layers, one mems case (B=3, L=50, mem_len 40: two segments, the second consuming the first one's cache)
and one query-stream case (B=4, L=50, M=5 targets; target_mapping / perm_mask come from query_stream_inputs below).  Run where the
reference checkout and transformers are available (the shim of oracle/make_golden.py; the reference's MAG takes its width from
modeling.TEXT_DIM, set around each build like VISUAL_DIM); asserts reference == oracle to 2e-5 and stores results only: inputs and weights
are regenerated from oracle/weights.py.  Full depth runs in about a minute on a CPU at these batches, L = 128 included.  SIZES, CASES,
MEMS_CASE, QS_CASE, size_config, key and query_stream_inputs are what the tests import."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (d_model, n_head, d_inner, n_layer)
SIZES = ((1024, 16, 4096, 24), (512, 8, 2048, 8), (256, 4, 1024, 4))
# (B, L, V, seed)
CASES = ((4, 50, 47, 11), (3, 128, 35, 13))
SAMPLE = 64
EXTRA_H, EXTRA_LAYERS = 1024, 2
MEMS_CASE = (3, 50, 40, 37)          # (B, L, mem_len, seed); segment 2 is the batch of seed + 100
QS_CASE = (4, 50, 5, 41)             # (B, L, M, seed)


def size_config(H, layers=None, num_labels=1):
    """keyword arguments of XLNetConfig / XLNetConfigLite for d_model H (layers: None = the full depth of SIZES)"""
    for (h, nh, inner, nl) in SIZES:
        if h == H:
            return dict(d_model=h, n_head=nh, d_inner=inner, n_layer=nl if layers is None else layers, num_labels=num_labels)
    raise KeyError(H)


def key(kind, H, B, L, V, seed):
    return "%s/H%d/B%d_L%d_V%d_seed%d" % (kind, H, B, L, V, seed)


def query_stream_inputs(mask, M, seed):
    """(target_mapping [B, M, L], perm_mask [B, L, L]) as float32 arrays: M one-hot targets per sample among its real tokens, hidden from
    every query (the targets themselves included: the g stream has no self exemption) -- the construction of oracle/make_golden.py"""
    mask = np.asarray(mask)
    B, L = mask.shape
    rs = np.random.RandomState(seed)
    tm = np.zeros((B, M, L), np.float32)
    pm = np.zeros((B, L, L), np.float32)
    for b in range(B):
        real = np.flatnonzero(mask[b] > 0)
        tgt = np.sort(rs.choice(real, size=M, replace=False))
        tm[b, np.arange(M), tgt] = 1.0
        pm[b][:, tgt] = 1.0
    return tm, pm


def main():
    from transformers.models.xlnet import configuration_xlnet as cx
    from oracle.make_golden import GOLD, MC, _load, _maxdiff, _tb, install_shim
    from oracle import mag_xlnet_ref as X
    from oracle import weights
    torch.manual_seed(0)
    cb, modeling, bert, xlnet = install_shim()
    out = {}

    def pair(H, layers, V):
        modeling.VISUAL_DIM = V
        xlnet.VISUAL_DIM = V
        modeling.TEXT_DIM = H
        try:
            kw = size_config(H, layers)
            ref = xlnet.MAG_XLNetForSequenceClassification(cx.XLNetConfig(mem_len=None, **kw), MC(1.0, 0.5))
        finally:
            modeling.VISUAL_DIM = 47
            xlnet.VISUAL_DIM = 47
            modeling.TEXT_DIM = 768
        _load(ref, "test")
        mine = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(**kw), X.MultimodalConfig(1.0, 0.5), V, 74)
        mine.load_state_dict(ref.state_dict(), strict=True)
        return ref.eval(), mine.eval()

    for (H, nh, inner, nl) in SIZES:
        for (B, L, V, seed) in CASES:
            ref, mine = pair(H, None, V)
            ids, vis, aco, mask, seg, lab = _tb(weights.synthetic_xlnet_batch(B, L, V, 74, seed=seed))
            with torch.no_grad():
                a = ref(ids, vis, aco, token_type_ids=seg, attention_mask=mask, labels=None)[0]
                sa = ref.transformer(ids, vis, aco, token_type_ids=seg, attention_mask=mask)[0]
                b = mine(ids, vis, aco, mask, seg)[0]
                sb = mine.transformer(ids, vis, aco, mask, seg)
            d, ds = _maxdiff(a, b), _maxdiff(sa, sb)
            print("G12 %d x %d/%d/%d B=%d L=%d V=%d seed=%d: reference vs oracle max |diff| logits %.3g, transformer output %.3g; logits %s"
                  % (nl, H, nh, inner, B, L, V, seed, d, ds, a.view(-1).tolist()))
            assert tuple(sa.shape) == (B, L, H) and d < 2e-5 and ds < 2e-5
            out[key("logits", H, B, L, V, seed)] = a.numpy()
            out[key("seq", H, B, L, V, seed)] = weights.strided_sample(sa.numpy(), SAMPLE)
            del ref, mine

    H = EXTRA_H
    ref, mine = pair(H, EXTRA_LAYERS, 47)
    # mems (as oracle/make_golden.py gen_xlnet): segment 1 caches, segment 2 consumes the cache and caches again
    B, L, ml, seed = MEMS_CASE
    ref.transformer.mem_len = ml
    b1, b2 = _tb(weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed)), _tb(weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed + 100))
    with torch.no_grad():
        r1 = ref(b1[0], b1[1], b1[2], token_type_ids=b1[4], attention_mask=b1[3], labels=None, use_cache=True)
        r2 = ref(b2[0], b2[1], b2[2], token_type_ids=b2[4], attention_mask=b2[3], labels=None, use_cache=True, mems=list(r1[1]))
        m1 = mine(b1[0], b1[1], b1[2], b1[3], b1[4], mem_len=ml)
        mems1 = mine.transformer.new_mems
        m2 = mine(b2[0], b2[1], b2[2], b2[3], b2[4], mems=mems1, mem_len=ml)
        mems2 = mine.transformer.new_mems
        no_mem = mine(b2[0], b2[1], b2[2], b2[3], b2[4])[0]
    d1, d2 = _maxdiff(r1[0], m1[0]), _maxdiff(r2[0], m2[0])
    dm1 = max(_maxdiff(a_, b_) for a_, b_ in zip(r1[1], mems1))
    dm2 = max(_maxdiff(a_, b_) for a_, b_ in zip(r2[1], mems2))
    print("G12 mems H=%d B=%d L=%d mem_len=%d: logits seg 1 / seg 2 max |diff| = %.3g / %.3g, new_mems %.3g / %.3g; the memory moves the "
          "segment-2 logits by %.3g" % (H, B, L, ml, d1, d2, dm1, dm2, _maxdiff(r2[0], no_mem)))
    assert max(d1, d2) < 2e-5 and max(dm1, dm2) < 2e-5 and tuple(r2[1][0].shape) == (min(ml, 2 * L), B, H)
    tag = "H%d/B%d_L%d_M%d_seed%d" % (H, B, L, ml, seed)
    out["mems/logits_seg1/" + tag] = r1[0].numpy()
    out["mems/logits_seg2/" + tag] = r2[0].numpy()
    for i in range(EXTRA_LAYERS):          # layer 0 = the embeddings, 1 = in front of the MAG injection
        out["mems/new_mems_seg1/%s/layer%d" % (tag, i)] = weights.strided_sample(r1[1][i].numpy(), SAMPLE)
        out["mems/new_mems_seg2/%s/layer%d" % (tag, i)] = weights.strided_sample(r2[1][i].numpy(), SAMPLE)
    ref.transformer.mem_len = None
    # the query stream under target_mapping
    B, L, M, seed = QS_CASE
    ids, vis, aco, mask, seg, lab = _tb(weights.synthetic_xlnet_batch(B, L, 47, 74, seed=seed))
    tm, pm = query_stream_inputs(mask.numpy(), M, seed)
    tm_t, pm_t = torch.from_numpy(tm), torch.from_numpy(pm)
    with torch.no_grad():
        a_g = ref.transformer(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t, target_mapping=tm_t)[0]
        b_g = mine.transformer(ids, vis, aco, mask, seg, perm_mask=pm_t, target_mapping=tm_t)
        a_l = ref(ids, vis, aco, token_type_ids=seg, attention_mask=mask, perm_mask=pm_t, target_mapping=tm_t, labels=None)[0]
        b_l = mine(ids, vis, aco, mask, seg, perm_mask=pm_t, target_mapping=tm_t)[0]
    dg, dl = _maxdiff(a_g, b_g), _maxdiff(a_l, b_l)
    print("G12 query stream H=%d B=%d L=%d M=%d: output_g max |diff| = %.3g (|g| max %.3g), logits %.3g" % (H, B, L, M, dg, float(a_g.abs().max()), dl))
    assert tuple(a_g.shape) == (B, M, H) and dg < 2e-5 and dl < 2e-5
    tag = "H%d/B%d_L%d_M%d_seed%d" % (H, B, L, M, seed)
    out["qs/output_g/" + tag] = weights.strided_sample(a_g.numpy(), SAMPLE)
    out["qs/logits/" + tag] = a_l.numpy()
    np.savez(os.path.join(GOLD, "g12_xlnet_sizes.npz"), **out)


if __name__ == "__main__":
    main()
