"""GPU: the LDS-resident attention kernels (csrc/attention.hip for MAG-BERT, csrc/xlnet_attention.hip for MAG-XLNet: every sequence of
up to 128 rows) at operator level against fp64 restatements of the same formulas on the CPU -- attn_op_helpers._xl_ref and
test_ops_gpu._attn_ref -- at the lengths where the padded length LP changes, below it (L < LP: the pad columns, the clamp of the
relative-position window, the row / column guards) and at it, with other head counts than 12, a perm mask, a fully padded sample,
NaN in everything the kernels own, and the query stream's fully masked rows.

Bounds: test_ops_gpu.close() times 2 for forward quantities and times 3 for backward ones, the factors of the tiled tests
(test_long_seq_gpu.py, test_xlnet_long_gpu.py).  B = 2 throughout; the fp64 references at L <= 128 take milliseconds."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import _lib
from attn_op_helpers import NAMES, _BertOp, _XlOp, _errors, xl_lp
from test_ops_gpu import DEV, DTS, close, stream


# ------------------------------------------------------------------------------------------------------------ MAG-XLNet
def _xl_check(case, what, backward=True, rerun=False):
    """one resident run of `case` against fp64: every output, every element; prints the measured errors; -> (got, ref_vec)"""
    dt, tdt, L = case.dt, case.tdt, case.L
    ref_vec, ref_grads = case.reference(backward=backward)
    got = case.run(tiled=False, backward=backward)
    for k, (e, s) in _errors(case, got, ref_vec, ref_grads).items():
        print("resident xlnet attention %s %s L=%d nh=%d %s: max|err| %.3e (max|ref| %.3e)" % (what, tdt, L, case.nh, k, e, s))
    vec, dqkv, dkr, pg = got
    for t in (vec, dqkv, dkr) + tuple(pg or ()):
        assert t is None or bool(torch.isfinite(t).all()), what
    close(vec.float(), ref_vec.float(), dt, what + " fwd", 2.0)
    if backward:
        close(dqkv.float(), ref_grads[0].float(), dt, what + " dq|dk|dv", 3.0)
        close(dkr.float(), ref_grads[1].float(), dt, what + " dkr", 3.0)
        for name, g, r in zip(NAMES[2:], pg, ref_grads[2:]):
            close(g, r.float().view(g.shape), dt, what + " " + name, 3.0)
    if rerun:              # vec, dqkv and dkr have one writer per element
        a, b = case.run(tiled=False), case.run(tiled=False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    return got, ref_vec


def _xl_check_psave(case, what):
    """the probabilities the last resident forward saved (before dropout), rows i < L: columns < L against the fp64 softmax, columns
    [L, LP) exact zeros"""
    B, L, nh, LP = case.B, case.L, case.nh, xl_lp(case.L)
    ps = case.psave.float().cpu().view(B, nh, LP, LP)
    e = float((ps[:, :, :L, :L].double() - case.ref_probs).abs().max())
    print("resident xlnet attention %s %s L=%d nh=%d psave: max|err| %.3e (max|ref| %.3e)" % (what, case.tdt, L, nh, e, float(case.ref_probs.max())))
    close(ps[:, :, :L, :L], case.ref_probs.float(), case.dt, what + " psave", 2.0)
    if L < LP:
        assert bool((ps[:, :, :L, L:] == 0.0).all()), what + ": psave columns >= L"


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [1, 7, 20, 32, 33, 50, 64, 65, 100, 127, 128])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_resident_relative_attention_vs_fp64(dt, tdt, L, p):
    """the three LP instantiations (32 | 64 | 128) at their lower edge, inside and at their upper edge, and the benchmark's L = 50; the
    key side of the backward is xl_attn_bwd_kv2 up to LP = 64 in bf16 and xl_attn_bwd_kv otherwise.  vec, dq | dk | dv, dkr, the four
    parameter gradients and the saved probabilities against fp64; row 0 at full length, row 1 left-padded down to 5 real keys (L = 1:
    no padding, L = 7: two padded keys), a head_scale with one zero, segment ids of both kinds; bit-identical reruns."""
    case = _XlOp(dt, tdt, 2, L, 12, 11, p)
    _xl_check(case, "p=%g" % p, rerun=True)
    _xl_check_psave(case, "p=%g" % p)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [20, 50, 100])
def test_resident_relative_attention_poisoned_scratch(dt, tdt, L):
    """psave, gsave, pdsave, vec, dqkv and dkr hold NaN before the forward (dropout on): the kernels write every element they own and
    read no scratch row or column >= L, so everything is finite and inside the same bounds"""
    case = _XlOp(dt, tdt, 2, L, 12, 13, 0.1, poison=True)
    _xl_check(case, "poisoned")
    _xl_check_psave(case, "poisoned")


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [50, 100])
@pytest.mark.parametrize("nh", [4, 8, 16])
def test_resident_relative_attention_head_counts(dt, tdt, L, nh):
    """d_model 256 / 512 / 1024: the row pitches 3 * nh * 64 and nh * 64 and the (batch, head) decomposition of the block index"""
    case = _XlOp(dt, tdt, 2, L, nh, 17, 0.1)
    _xl_check(case, "heads")
    _xl_check_psave(case, "heads")


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [20, 50, 100])
def test_resident_relative_attention_perm_mask(dt, tdt, L):
    """a random perm (30 %) next to the padding, dropout on: the backward works from psave, so this is the forward's perm reaching it"""
    case = _XlOp(dt, tdt, 2, L, 12, 23, 0.1, perm=True)
    _xl_check(case, "perm")
    _xl_check_psave(case, "perm")


@pytest.mark.parametrize("dt,tdt", DTS)
def test_resident_relative_attention_fully_padded_sample(dt, tdt):
    """mask[1, :] = 0 at L = 50: with the i == j exemption every row of sample 1 attends to itself only (the reference says so: its
    probabilities are the identity), and the kernels agree with fp64 in every output"""
    case = _XlOp(dt, tdt, 2, 50, 12, 29, 0.1, padded_sample=True)
    _xl_check(case, "padded sample")
    assert torch.equal(case.ref_probs[1], torch.eye(50, dtype=torch.float64).expand(12, 50, 50))
    _xl_check_psave(case, "padded sample")


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("L", [20, 50, 100])
def test_resident_query_stream_fully_masked_row(dt, tdt, L):
    """gstream = 1 (no self exemption), forward only: a row whose every key carries -1e30 is the uniform average of the L value rows
    times head_scale -- the LP - L padding columns weigh nothing.  The whole output against fp64, those rows included."""
    case = _XlOp(dt, tdt, 2, L, 12, 31, 0.0, gstream=1)
    (vec, _, _, _), ref_vec = _xl_check(case, "gstream", backward=False)
    for b, i in ((0, L // 2), (1, L - 2)):
        v = case.qkv.double().view(2, L, 3, 12, 64)[b, :, 2].mean(0) * case.hs.double()[:, None]          # uniform over all L keys
        row = vec.float().cpu().view(2, L, 12, 64)[b, i]
        print("resident xlnet attention gstream %s L=%d fully masked row (%d, %d): max|err| %.3e (max|ref| %.3e)"
              % (tdt, L, b, i, float((row.double() - v).abs().max()), float(v.abs().max())))
        close(row, v.float(), dt, "fully masked row (%d, %d)" % (b, i), 2.0)


# ------------------------------------------------------------------------------------------------------------ MAG-BERT
def _bert_plain(dt, tdt, S, nh, p, mask, what):
    """mb_attention_forward / _backward (NaN in both outputs before the calls): ctx and dqkv against fp64"""
    c = _BertOp(dt, tdt, S, nh, p, mask)
    L, H = _lib.lib(), nh * 64
    out = torch.full((2 * S, H), float("nan"), dtype=tdt, device=DEV)
    dq = torch.full((2 * S, 3 * H), float("nan"), dtype=tdt, device=DEV)
    _lib.check(L.mb_attention_forward(dt, _lib.ptr(c.qd), _lib.ptr(c.md), _lib.ptr(out), 2, S, nh, c.kp, stream()))
    _lib.check(L.mb_attention_backward(dt, _lib.ptr(c.qd), _lib.ptr(c.md), _lib.ptr(c.dcd), _lib.ptr(dq), 2, S, nh, c.kp, stream()))
    torch.cuda.synchronize()
    c.errors(what, ctx=out, dqkv=dq)
    return c


def _bert_mask(S):
    mask = torch.ones(2, S, dtype=torch.long)
    mask[1, 3:] = 0                                                      # row 0 at full length, row 1 nearly all padding
    return mask


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("S", [1, 31, 32, 33, 64, 65, 97, 127])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_resident_bert_attention_lp_boundaries(dt, tdt, S, p):
    """the four LP instantiations (32 | 64 | 96 | 128) at and next to their edges, a single token"""
    _bert_plain(dt, tdt, S, 12, p, _bert_mask(S), "p=%g" % p)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("nh", [4, 8, 16])
def test_resident_bert_attention_head_counts(dt, tdt, nh):
    """hidden sizes 256 / 512 / 1024 at S = 50"""
    _bert_plain(dt, tdt, 50, nh, 0.1, _bert_mask(50), "heads")


@pytest.mark.parametrize("dt,tdt", DTS)
def test_resident_bert_attention_fully_padded_sample(dt, tdt):
    """mask[1, :] = 0 at S = 50: the additive -10000 is the same for every key, so the reference is the unmasked softmax.

    Adding the -10000 as it stands costs fp32 half an ulp of 10000, 4.9e-4, in every score of such a sample (measured: ctx 3.8e-4
    against a bound of 6.2e-5, dqkv 3.0e-4 against 1.0e-4), so the kernels take the bias that all keys of a sample share off before
    they add it (attention.hip common_key_bias): ctx 9.5e-7, dqkv 7.2e-7 in fp32, 6.9e-3 / 6.9e-3 in bf16."""
    mask = torch.ones(2, 50, dtype=torch.long)
    mask[1, :] = 0
    c = _bert_plain(dt, tdt, 50, 12, 0.1, mask, "padded sample")
    q, k, _ = c.qkv.detach().double().view(2, 50, 3, 12, 64).permute(2, 0, 3, 1, 4)
    assert float((c.soft[1] - torch.softmax(q[1] @ k[1].transpose(-1, -2) / 8.0, -1)).abs().max()) <= 1e-12


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("S", [20, 50, 96, 128])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_resident_attention_vs_fp64(dt, tdt, S, p):
    """test_long_seq_gpu.test_tiled_attention_vs_fp64 for the LDS-resident kernels (mb_attention_resident_forward / _backward): a
    head_scale with one zero, the probabilities after dropout and head mask, the fused QKV bias gradient against the column sums of
    the fp64 dqkv, bit-identical dqkv on reruns without dbias"""
    nh = 12
    H = nh * 64
    mask = torch.ones(2, S, dtype=torch.long)
    mask[0, S - 7:] = 0
    mask[1, 3:] = 0                                                      # nearly everything padded
    hs = torch.linspace(0.5, 1.5, nh, dtype=torch.float32)
    hs[3] = 0.0
    c = _BertOp(dt, tdt, S, nh, p, mask, hs)
    L = _lib.lib()

    def run(probs, dbias):
        out = torch.zeros(2 * S, H, dtype=tdt, device=DEV)
        pr = torch.zeros(2, nh, S, S, dtype=torch.float32, device=DEV) if probs else None
        _lib.check(L.mb_attention_resident_forward(dt, _lib.ptr(c.qd), _lib.ptr(c.md), _lib.ptr(out), 2, S, nh, c.kp, _lib.ptr(c.hsd),
                                                   _lib.ptr(pr), stream()))
        dq = torch.zeros(2 * S, 3 * H, dtype=tdt, device=DEV)
        db = torch.zeros(3 * H, dtype=torch.float32, device=DEV) if dbias else None
        _lib.check(L.mb_attention_resident_backward(dt, _lib.ptr(c.qd), _lib.ptr(c.md), _lib.ptr(c.dcd), _lib.ptr(dq), _lib.ptr(db), 2, S,
                                                    nh, c.kp, _lib.ptr(c.hsd), stream()))
        torch.cuda.synchronize()
        return out, dq, pr, db
    out, dq, pr, db = run(True, True)
    c.errors("p=%g head_scale" % p, ctx=out, probs=pr, dqkv=dq, dbias=db)
    assert torch.equal(run(False, False)[1], run(False, False)[1])
    with pytest.raises(_lib.MagbertError):
        _lib.check(L.mb_attention_resident_forward(dt, _lib.ptr(c.qd), _lib.ptr(c.md), _lib.ptr(out), 2, 129, nh, c.kp, None, None, stream()))
