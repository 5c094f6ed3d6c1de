"""GPU: the tiled attention kernels (csrc/attention_tiled.hip for MAG-BERT, csrc/xlnet_attention_tiled.hip for MAG-XLNet: every
sequence longer than 128 rows, and callable from 1) at operator level against fp64 restatements of the same formulas on the CPU --
test_ops_gpu._attn_ref and attn_op_helpers._xl_ref -- at the lengths next to the 64-row block edges (below one block, one row into the
next block, odd and even tile counts), with other head counts than 12, masks that blank whole key tiles for a whole query block
(left padding, holes, a perm block), a fully padded sample, a third sample with an odd number of blocks per sequence, and NaN in
everything the kernels own or pass between their launches.

Bounds: test_ops_gpu.close() times 2 for forward quantities and times 3 for backward ones, the factors of test_long_seq_gpu.py,
test_xlnet_long_gpu.py and test_attention_resident_gpu.py.  nh = 4, B = 2 and dropout 0.1 unless the case is about something else; a
head_scale with one zero throughout.  The case lists (BERT_CASES / XL_CASES) are plain data, so the fp64 references can be run alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import _lib
from attn_op_helpers import NAMES, _BertOp, _XlOp, _errors, _tiled
from test_ops_gpu import DEV, DTS, close, stream

EDGES = [1, 7, 63, 65, 127, 130, 191, 192, 193, 257, 320, 449, 511]
P = 0.1


def _head_scale(nh):
    hs = torch.linspace(0.5, 1.5, nh, dtype=torch.float32)
    hs[3] = 0.0
    return hs


# ------------------------------------------------------------------------------------------------------------ MAG-BERT
def bert_mask(kind, S, B=2):
    mask = torch.ones(B, S, dtype=torch.long)
    if kind == "edge":                                # row 0 at full length, row 1 with three real keys (S = 1: no padding)
        if S > 1:
            mask[1, 3:] = 0
    elif kind == "left":                              # the first key tiles of sample 1 entirely masked
        mask[1, :S - 5] = 0
    elif kind == "holes":                             # every third key of sample 0, key 0 among them
        mask[0, ::3] = 0
    elif kind == "left+holes":
        mask[1, :S - 5] = 0
        mask[0, ::3] = 0
    elif kind == "padded":                            # sample 1 has no real key at all
        mask[1, :] = 0
    elif kind == "three":                             # B = 3: row 2 left-padded past its first key tile, and a short right pad
        mask[1, 3:] = 0
        mask[2, :66] = 0
        mask[2, S - 2:] = 0
    else:
        raise ValueError(kind)
    return mask


def bert_case(dt, tdt, kind, S, nh=4, B=2, dev=DEV):
    return _BertOp(dt, tdt, S, nh, P, bert_mask(kind, S, B), _head_scale(nh), family="tiled", dev=dev)


def _bert_run(c, **kw):
    return _tiled(c.dt, c.tdt, c.qd, c.md, c.dcd, c.B, c.S, c.nh, c.key, c.hsd, **kw)


def _bert_check(c, what, poison=False, resident=False):
    """one tiled forward + backward with probs and dbias against fp64: every output, every element; prints the measured errors"""
    out, dq, pr, db = _bert_run(c, probs=True, dbias=True, poison=poison)
    for name, t in (("ctx", out), ("probs", pr), ("dqkv", dq), ("dbias", db)):
        assert bool(torch.isfinite(t).all()), what + " " + name
    c.errors(what, ctx=out, probs=pr, dqkv=dq, dbias=db)
    if resident:                                      # the LDS-resident pair on the same inputs (same dropout key, same head_scale)
        L, (B, S, nh) = _lib.lib(), (c.B, c.S, c.nh)
        r_out = torch.zeros_like(out)
        r_dq = torch.zeros_like(dq)
        _lib.check(L.mb_attention_resident_forward(c.dt, _lib.ptr(c.qd), _lib.ptr(c.md), _lib.ptr(r_out), B, S, nh, c.kp, _lib.ptr(c.hsd),
                                                   None, stream()))
        _lib.check(L.mb_attention_resident_backward(c.dt, _lib.ptr(c.qd), _lib.ptr(c.md), _lib.ptr(c.dcd), _lib.ptr(r_dq), None, B, S, nh,
                                                    c.kp, _lib.ptr(c.hsd), stream()))
        torch.cuda.synchronize()
        for name, g, r in (("ctx", out, r_out), ("dqkv", dq, r_dq)):
            print("tiled bert attention %s vs resident %s S=%d nh=%d %s: max|diff| %.3e (max|ref| %.3e)"
                  % (what, c.tdt, S, nh, name, float((g.float() - r.float()).abs().max()), float(r.float().abs().max())))
        close(out.float(), r_out.float().cpu(), c.dt, what + " tiled vs resident ctx", 2.0)
        close(dq.float(), r_dq.float().cpu(), c.dt, what + " tiled vs resident dqkv", 3.0)


def _assert_padded_reference(c):
    """the additive -10000 is the same for every key of sample 1, so the fp64 reference of that sample is the unmasked softmax"""
    q, k, _ = c.qkv.detach().double().view(c.B, c.S, 3, c.nh, 64).permute(2, 0, 3, 1, 4)
    assert float((c.soft[1] - torch.softmax(q[1] @ k[1].transpose(-1, -2) / 8.0, -1)).abs().max()) <= 1e-12


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("S", EDGES)
def test_tiled_bert_attention_block_edges(dt, tdt, S):
    """below one 64-row block, one row into the next, around odd and even tile counts: the `valid` row guards of TileStage, the kPadNeg
    columns of the last key tile, the rows >= L of the last query block; at S <= 128 also against the LDS-resident pair"""
    _bert_check(bert_case(dt, tdt, "edge", S), "edges", resident=S <= 128)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("S", [130, 300])
@pytest.mark.parametrize("kind", ["left", "holes", "left+holes"])
def test_tiled_bert_attention_mask_shapes(dt, tdt, S, kind):
    """left padding: the online softmax of sample 1 starts from m ~ -10000 on key tiles that are entirely masked and must rescale them
    to nothing once a real key arrives; holes: masked keys inside every tile, key 0 among them"""
    _bert_check(bert_case(dt, tdt, kind, S), kind)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("S", [100, 200, 512])
def test_tiled_bert_attention_fully_padded_sample(dt, tdt, S):
    """mask[1, :] = 0: the reference is the unmasked softmax (asserted).  Adding the -10000 as it stands costs fp32 half an ulp of
    10000, 4.9e-4, in every score of such a sample, so the kernels take the bias common to all keys of a sample off first
    (attn_common.h common_key_bias), as the resident ones do.  fp32, measured with the library before that -> with it (bound):
        S = 100: ctx 3.57e-04 -> 6.6e-07 (5.3e-05)   probs 1.37e-04 -> 2.5e-07 (2.7e-05)   dqkv 2.50e-04 -> 5.4e-07 (7.3e-05)
        S = 200: ctx 2.35e-04 -> 8.3e-07 (4.3e-05)   probs 9.86e-05 -> 2.5e-07 (1.8e-05)   dqkv 2.01e-04 -> 7.2e-07 (5.9e-05)
        S = 512: ctx 2.20e-04 -> 9.5e-07 (3.2e-05)   probs 9.50e-05 -> 3.9e-07 (1.6e-05)   dqkv 1.51e-04 -> 7.7e-07 (4.0e-05)
    (dbias 1.1e-03 ... 1.2e-03 -> 2.5e-06 ... 6.9e-06, inside its bound either way).  bf16: ctx and dqkv at their own rounding before and after (5.5e-03 / 4e-03 at S = 100), probs (an
    fp32 output) 1.1e-04 -> 8e-08; inside the bf16 bounds either way."""
    c = bert_case(dt, tdt, "padded", S)
    _assert_padded_reference(c)
    _bert_check(c, "padded sample", resident=S <= 128)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("nh", [8, 12, 16])
def test_tiled_bert_attention_head_counts(dt, tdt, nh):
    """hidden sizes 512 / 768 / 1024 at S = 200: the row pitches 3 * nh * 64 and nh * 64, the (batch, head, block) decomposition"""
    _bert_check(bert_case(dt, tdt, "edge", 200, nh=nh), "heads")


@pytest.mark.parametrize("dt,tdt", DTS)
def test_tiled_bert_attention_three_samples_odd_blocks(dt, tdt):
    """B = 3, S = 130: three blocks per sequence, a batch index of 2 out of blockIdx.x / nqb"""
    _bert_check(bert_case(dt, tdt, "three", 130, B=3), "B=3")


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("S", [130, 200])
def test_tiled_bert_attention_poisoned_outputs_and_stats(dt, tdt, S):
    """ctx, probs, dqkv and the three stats planes hold NaN before the forward: the kernels write every element they own and read no
    statistic they have not written, so everything is finite and inside the same bounds"""
    _bert_check(bert_case(dt, tdt, "edge", S), "poisoned", poison=True)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("kind,S", [("edge", 193), ("padded", 200)])
def test_tiled_bert_attention_reruns_are_bit_identical(dt, tdt, kind, S):
    """without dbias every dQ / dK / dV element has one writer"""
    c = bert_case(dt, tdt, kind, S)
    a, b = _bert_run(c), _bert_run(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------ MAG-XLNet
def xl_perm_blocks(B, L):
    """blanks whole 64 x 64 tiles: the first key tile of query block 1, every tile but the first of query block 0 of sample 0.  With
    gstream = 0 the diagonal exemption keeps every row alive"""
    perm = torch.zeros(B, L, L, dtype=torch.uint8)
    perm[:, 64:128, 0:64] = 1
    perm[0, 0:64, 64:] = 1
    return perm


def xl_case(dt, tdt, kind, L, nh=4, dev=DEV):
    seed = {"edges": 11, "poisoned": 13, "heads": 17, "padded sample": 29, "perm blocks": 23}[kind]
    return _XlOp(dt, tdt, 2, L, nh, seed, P, perm=xl_perm_blocks(2, L) if kind == "perm blocks" else False, poison=kind == "poisoned",
                 padded_sample=kind == "padded sample", dev=dev)


def _xl_check(case, what, rerun=False, resident=False):
    """one tiled run of `case` against fp64: every output, every element; prints the measured errors"""
    dt, tdt, L = case.dt, case.tdt, case.L
    ref_vec, ref_grads = case.reference()
    got = case.run(tiled=True)
    for k, (e, s) in _errors(case, got, ref_vec, ref_grads).items():
        print("tiled xlnet attention %s %s L=%d nh=%d %s: max|err| %.3e (max|ref| %.3e)" % (what, tdt, L, case.nh, k, e, s))
    vec, dqkv, dkr, pg = got
    for t in (vec, dqkv, dkr) + tuple(pg):
        assert bool(torch.isfinite(t).all()), what
    close(vec.float(), ref_vec.float(), dt, what + " fwd", 2.0)
    close(dqkv.float(), ref_grads[0].float(), dt, what + " dq|dk|dv", 3.0)
    close(dkr.float(), ref_grads[1].float(), dt, what + " dkr", 3.0)
    for name, g, r in zip(NAMES[2:], pg, ref_grads[2:]):
        close(g, r.float().view(g.shape), dt, what + " " + name, 3.0)
    if rerun:              # vec, dqkv and dkr have one writer per element
        a, b = case.run(tiled=True), case.run(tiled=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    if resident:           # the LDS-resident kernels on the same inputs
        r = case.run(tiled=False)
        for name, g, x in zip(("vec", "dqkv", "dkr"), got[:3], r[:3]):
            print("tiled xlnet attention %s vs resident %s L=%d nh=%d %s: max|diff| %.3e (max|ref| %.3e)"
                  % (what, tdt, L, case.nh, name, float((g.float() - x.float()).abs().max()), float(x.float().abs().max())))
        close(vec.float(), r[0].float().cpu(), dt, what + " tiled vs resident fwd", 2.0)
        close(dqkv.float(), r[1].float().cpu(), dt, what + " tiled vs resident dq|dk|dv", 3.0)
        close(dkr.float(), r[2].float().cpu(), dt, what + " tiled vs resident dkr", 3.0)
        for name, g, x in zip(NAMES[2:], pg, r[3]):
            close(g, x.cpu(), dt, what + " tiled vs resident " + name, 3.0)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", EDGES)
def test_tiled_relative_attention_block_edges(dt, tdt, L):
    """the row guards of XTileStage, the -inf columns of the last key tile, the three-slot kr window (L - i0 - 63 + j0) at its clamps and
    the bwd_pos blocks over 2L position rows; row 0 at full length, row 1 left-padded down to 5 real keys (its first key tiles are
    entirely masked); bit-identical reruns; at L <= 128 also against the LDS-resident kernels"""
    _xl_check(xl_case(dt, tdt, "edges", L), "edges", rerun=True, resident=L <= 128)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [130, 200, 449])
def test_tiled_relative_attention_poisoned_scratch(dt, tdt, L):
    """vec, dqkv, dkr and the two [B * nh][LP][LP] planes the three backward launches pass G and Pd through hold NaN before the forward:
    no launch reads a row or column >= L of a plane (NaN times a zero operand inside an MFMA is NaN)"""
    _xl_check(xl_case(dt, tdt, "poisoned", L), "poisoned")


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("nh", [8, 16])
def test_tiled_relative_attention_head_counts(dt, tdt, nh):
    """d_model 512 / 1024 at L = 200"""
    _xl_check(xl_case(dt, tdt, "heads", 200, nh=nh), "heads")


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [200, 449])
def test_tiled_relative_attention_fully_padded_sample(dt, tdt, L):
    """mask[1, :] = 0: with the i == j exemption every row of sample 1 attends to itself only (the reference says so: its
    probabilities are the identity), every key tile off the diagonal is entirely masked.

    The true score gradient of such a row is exactly zero, and all the diagonals land on the one position row dkr[L].  While the bf16
    backward took D_i = dvec_i . vec_i from the rounded vec, dkr measured 7.3e-02 at L = 200 and 1.5e-01 at L = 449 (bounds 3.5e-02 /
    3.8e-02; block_edges at L = 1, where dkr is zero: 7.8e-03 against 3e-06); with D_i summed from the probabilities in fp32
    (xl_tiled_bwd_q_kernel) 3.8e-03 / 3.8e-03 and 1.2e-07."""
    case = xl_case(dt, tdt, "padded sample", L)
    _xl_check(case, "padded sample")
    assert torch.equal(case.ref_probs[1], torch.eye(L, dtype=torch.float64).expand(case.nh, L, L))


@pytest.mark.parametrize("dt,tdt", DTS)
def test_tiled_relative_attention_perm_blanks_whole_tiles(dt, tdt):
    """L = 200: query block 1 meets an entirely masked first key tile (the online softmax starts from m = -1e30 and must rescale to
    nothing), query block 0 of sample 0 only masked tiles after its first"""
    _xl_check(xl_case(dt, tdt, "perm blocks", 200), "perm blocks")
