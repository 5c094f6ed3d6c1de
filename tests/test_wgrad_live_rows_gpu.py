"""GPU: the gathered k loop of the 256 x 128 ping-pong grouped weight gradient (csrc/gemm_pp.hip gemm_pp_grouped_tn_gather_kernel, through
the test hook mb_debug_gemm_grouped_rows) and the live-row list the step prologue builds for it (csrc/rowops.hip live_rows_block, through
mb_debug_live_rows).

Operator: dW_g (+)= sum over the listed rows r of dY_g[r]^T X_g[r].  Two problems per launch -- one tile (256 x 128) and 512 x 256, which
crosses the 128-row seam between the two wave groups -- with DIFFERENT lists; Tp = 256 and 320 rows; lists of 1, 48, 191, 192, 193, 255,
256 and Tp rows (the 3-stage minimum, the pad-to-64 rule, the identity list), with gaps and ending on the last row.  Every row that is
neither listed nor the pad row is NaN in both operands, so a single read of it shows in the output; the pad row is zero in dY and random
in X.  Reference: fp64 over the listed rows; bound (tests/gemm_op_helpers.py, fp32 outputs): n 2^-24 |dY|^T |X| + 2^-24 (|init| + |ref|)
per element, n = the length of the list as the kernel sums it (padding included) -- the worst case of any fp32 summation order of n
exact products plus the rounding of the store.  The identity list must give the bits of the dense launch.

Prologue: the live-row list and the [CLS]-row list of a mask against a numpy twin, which is itself checked against lists written out by
hand; masks: all live, all dead, one live row, non-prefix, live tokens behind a [CLS] row whose own word is 0, one fully padded sample."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import _lib

import gemm_op_helpers as H

DEV = "cuda:0"
SHAPES = [(256, 128), (512, 256)]
COUNTS = [1, 48, 191, 192, 193, 255, 256, None]          # None: Tp (the identity list)
GATHER_SYM = "gemm_pp_grouped_tn_gather_kernel"


def _list(Tp, count, seed):
    """`count` ascending rows of [0, Tp) that end on the last row and leave gaps -> (live rows, pad row or None, the list as the kernel gets it)"""
    if count >= Tp:
        live = np.arange(Tp)
    else:
        g = np.random.default_rng(seed)
        live = np.sort(np.concatenate([g.choice(Tp - 1, size=count - 1, replace=False), [Tp - 1]])).astype(np.int64)
    n = max(192, -(-len(live) // 64) * 64)
    pad = None
    if n > len(live):
        pad = int(np.setdiff1d(np.arange(Tp), live)[0])
    full = np.concatenate([live, np.full(n - len(live), pad if pad is not None else 0)]).astype(np.uint32)
    return live, pad, full


def _operand(Tp, cols, live, seed, tdt, scale):
    """-> (values [Tp][cols], allocation [Tp + guard][cols + 8]: the values on the listed rows, NaN everywhere else)"""
    x = H.rnd((Tp, cols), seed, tdt, scale)
    buf = torch.full((Tp + H.GUARD, cols + 8), float("nan"), dtype=tdt)
    buf[live, :cols] = x[live].to(tdt)
    return x, buf


def _launch(L, probs, K, rows, nrows, gathered):
    n = len(probs)
    Ms, Ns = [p["M"] for p in probs], [p["N"] for p in probs]
    args = [H.BF16, n, H._int_arr(Ms), H._int_arr(Ns), K, H._ptr_arr([p["dY_d"].data_ptr() for p in probs]),
            H._int_arr([p["dY_d"].shape[1] for p in probs]), H._ptr_arr([p["X_d"].data_ptr() for p in probs]),
            H._int_arr([p["X_d"].shape[1] for p in probs]), H._ptr_arr([p["W_d"].data_ptr() for p in probs]),
            H._int_arr([p["N"] + 8 for p in probs])]
    if gathered:
        rc = L.mb_debug_gemm_grouped_rows(*args, H._int_arr([0] * n), 256, H._ptr_arr([r.data_ptr() if r is not None else None for r in rows]),
                                          H._ptr_arr([c.data_ptr() if c is not None else None for c in nrows]), H._stream())
    else:
        rc = L.mb_debug_gemm_grouped_ex(*args, H._int_arr([0] * n), H._int_arr([0] * n), 256, 0, *H._ride_args(None), H._stream())
    torch.cuda.synchronize()
    return rc


def _problems(Tp, counts, seed):
    tdt = torch.bfloat16
    probs = []
    for i, ((M, N), count) in enumerate(zip(SHAPES, counts)):
        live, pad, full = _list(Tp, count if count is not None else Tp, seed + 7 * i)
        dY, dY_buf = _operand(Tp, M, live, seed + 10 * i + 1, tdt, 1.0)
        X, X_buf = _operand(Tp, N, live, seed + 10 * i + 2, tdt, 0.1)
        if pad is not None:
            dY_buf[pad, :M] = 0.0
            X_buf[pad, :N] = X[pad].to(tdt)                # finite, and multiplied by the zero row only
        init = H.rnd((M, N), seed + 10 * i + 3, torch.float32)
        W = H.canary(((M + H.GUARD) * (N + 8),), torch.float32)
        W[:M * (N + 8)].view(M, N + 8)[:, :N] = init
        probs.append(dict(M=M, N=N, live=live, pad=pad, full=full, dY=dY, X=X, init=init, W=W, dY_d=dY_buf.to(DEV), X_d=X_buf.to(DEV),
                          rows_d=torch.from_numpy(full.astype(np.int32)).to(DEV), n_d=torch.tensor([len(full)], dtype=torch.int32, device=DEV)))
    return probs


def _check(p, got, what):
    M, N = p["M"], p["N"]
    Y, X = p["dY"][p["live"]].double(), p["X"][p["live"]].double()
    ref = p["init"].double() + Y.t() @ X
    bound = len(p["full"]) * 2.0 ** -24 * (Y.abs().t() @ X.abs()) + 2.0 ** -24 * (p["init"].double().abs() + ref.abs()) + H.TINY
    img = got[:M * (N + 8)].view(M, N + 8)
    own = torch.zeros(got.shape, dtype=torch.bool)
    own[:M * (N + 8)].view(M, N + 8)[:, :N] = True
    assert bool(H.is_canary(got)[~own].all()), what + ": written outside the output"
    out = img[:, :N].double()
    assert bool(torch.isfinite(out).all()), what + ": %d non-finite outputs (a row outside the list was read)" % int((~torch.isfinite(out)).sum())
    ratio = ((out - ref).abs() / bound).max()
    print("%s: worst |err| / bound %.3f" % (what, float(ratio)))
    assert float(ratio) <= 1.0, "%s: |err| / bound %.3f" % (what, float(ratio))


@pytest.mark.parametrize("Tp", [256, 320])
@pytest.mark.parametrize("ci", range(len(COUNTS)))
def test_gathered_wgrad(Tp, ci):
    L = _lib.lib()
    # the two problems of the launch take different lists: this count and the next one of the table
    counts = (COUNTS[ci], COUNTS[(ci + 3) % len(COUNTS)])
    probs = _problems(Tp, counts, 1000 * Tp + 50 * ci)
    for p in probs:
        p["W_d"] = p["W"].to(DEV)
    rc = _launch(L, probs, Tp, [p["rows_d"] for p in probs], [p["n_d"] for p in probs], True)
    assert rc == 0, "rc %d" % rc
    assert GATHER_SYM in H.last_kernel(), H.last_kernel()
    outs = [p["W_d"].cpu() for p in probs]
    for i, p in enumerate(probs):
        _check(p, outs[i], "Tp %d problem %d (%d x %d) rows %d" % (Tp, i, p["M"], p["N"], len(p["live"])))


@pytest.mark.parametrize("Tp", [256, 320])
def test_identity_list_is_dense(Tp):
    """the list 0 .. Tp-1 sums the same rows in the same order as the dense loop: the same bits; a launch that mixes a listed and an
    unlisted (dense) problem runs both in the gathered kernel"""
    L = _lib.lib()
    probs = _problems(Tp, (None, None), 77 + Tp)
    res = []
    for mode in ("dense", "rows", "mixed"):
        for p in probs:
            p["W_d"] = p["W"].to(DEV)
        rows = [p["rows_d"] for p in probs]
        cnt = [p["n_d"] for p in probs]
        if mode == "mixed":
            rows[1] = cnt[1] = None
        assert _launch(L, probs, Tp, rows, cnt, mode != "dense") == 0
        sym = H.last_kernel()
        assert (GATHER_SYM in sym) == (mode != "dense"), (mode, sym)
        if mode == "dense":
            assert H.kernel_key(sym) == "ppgrp:256x128:3:128", sym
        res.append([p["W_d"].cpu().view(torch.int32) for p in probs])
    for i in range(len(probs)):
        assert torch.equal(res[0][i], res[1][i]), "problem %d: the identity list differs from the dense launch" % i
        assert torch.equal(res[0][i], res[2][i]), "problem %d: mixed launch differs from the dense launch" % i
        _check(probs[i], res[1][i].view(torch.float32), "identity Tp %d problem %d" % (Tp, i))


def test_rows_need_the_pingpong_tile():
    """a list handed to any other grouped kernel is refused, not run dense"""
    L = _lib.lib()
    probs = _problems(256, (192, 192), 5)
    for p in probs:
        p["W_d"] = p["W"].to(DEV)
    n = len(probs)
    rc = L.mb_debug_gemm_grouped_rows(H.BF16, n, H._int_arr([p["M"] for p in probs]), H._int_arr([p["N"] for p in probs]), 256,
                                      H._ptr_arr([p["dY_d"].data_ptr() for p in probs]), H._int_arr([p["dY_d"].shape[1] for p in probs]),
                                      H._ptr_arr([p["X_d"].data_ptr() for p in probs]), H._int_arr([p["X_d"].shape[1] for p in probs]),
                                      H._ptr_arr([p["W_d"].data_ptr() for p in probs]), H._int_arr([p["N"] + 8 for p in probs]),
                                      H._int_arr([0] * n), 128, H._ptr_arr([p["rows_d"].data_ptr() for p in probs]),
                                      H._ptr_arr([p["n_d"].data_ptr() for p in probs]), H._stream())
    torch.cuda.synchronize()
    assert rc == H.MB_ERR_MODE, rc


# ------------------------------------------------------------------------------------------------ the prologue's lists
def _expected_list(mask, Tp):
    """numpy twin of live_rows_block.  Live: a row whose mask word is set; row 0 of EVERY sample (the head reads hidden[:, 0] and attention
    masks keys, not queries: the [CLS] row has a gradient whatever its mask word); every row of a sample with no set word at all (its
    softmax runs over all its keys).  -> (live list, its count, live map, [CLS] list, its count)"""
    B, L = mask.shape
    T = B * L
    real = mask.any(axis=1)
    lm = (mask != 0) | ~real[:, None]
    lm[:, 0] = True
    live_map = lm.reshape(-1)
    live = np.nonzero(live_map)[0]
    dead = np.nonzero(~live_map)[0]
    have_pad = len(dead) > 0 or T < Tp
    pad = int(dead[0]) if len(dead) else (T if T < Tp else 0)
    count = max(192, -(-len(live) // 64) * 64)
    full = np.concatenate([live, np.full(count - len(live), pad)]).astype(np.uint32)
    if have_pad:
        cc = max(192, -(-B // 64) * 64)
        cls = np.concatenate([np.arange(B) * L, np.full(cc - B, pad)]).astype(np.uint32)
    else:
        cc, cls = count, full
    return full, count, live_map, cls, cc


def _masks(B, L):
    g = np.random.default_rng(B * 100 + L)
    out = {"all_live": np.ones((B, L), np.int64), "all_dead": np.zeros((B, L), np.int64)}
    one = np.zeros((B, L), np.int64)
    one[1, 3] = 1
    out["one_live_row"] = one
    out["non_prefix"] = (g.random((B, L)) < 0.5).astype(np.int64)
    out["non_prefix"][:, 0] = 1
    dead_cls = (g.random((B, L)) < 0.5).astype(np.int64)          # live tokens behind a [CLS] row whose own mask word is 0
    dead_cls[:, 0] = 0
    dead_cls[:, 2] = 1
    out["dead_cls_word"] = dead_cls
    pref = (np.arange(L)[None, :] < g.integers(3, L, size=(B, 1))).astype(np.int64)
    pref[B - 1, :] = 0
    out["one_padded_sample"] = pref
    last = np.ones((B, L), np.int64)
    last[0, 1:] = 0
    out["dead_rows_in_sample_0"] = last
    return out


def test_expected_list_by_hand():
    """the twin itself, against lists written out by hand (B = 3, L = 4, Tp = 64: row 12 is the first zero pad row)"""
    m = np.array([[0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0]], np.int64)
    full, count, live_map, cls, cc = _expected_list(m, 64)
    # sample 0 has no set word: whole; sample 1: its [CLS] row 4 although mask[1][0] == 0, and row 6; sample 2: rows 8, 9
    assert list(np.nonzero(live_map)[0]) == [0, 1, 2, 3, 4, 6, 8, 9]
    assert count == 192 and list(full[:9]) == [0, 1, 2, 3, 4, 6, 8, 9, 5] and bool((full[8:] == 5).all())
    assert cc == 192 and list(cls[:4]) == [0, 4, 8, 5] and bool((cls[3:] == 5).all())


@pytest.mark.parametrize("B,L", [(3, 50), (4, 16)])
def test_prologue_lists(B, L):
    lib = _lib.lib()
    T = B * L
    Tp = -(-T // 64) * 64
    cap = max(192, Tp)
    for name, mask in _masks(B, L).items():
        bufs = [torch.full((cap + 8,), 0x7FFFFFFF, dtype=torch.int32, device=DEV) for _ in range(2)]
        cnts = [torch.full((1,), -1, dtype=torch.int32, device=DEV) for _ in range(2)]
        m = torch.from_numpy(mask).to(DEV)
        rc = lib.mb_debug_live_rows(_lib.ptr(m), B, L, Tp, _lib.ptr(bufs[0]), _lib.ptr(cnts[0]), _lib.ptr(bufs[1]), _lib.ptr(cnts[1]), H._stream())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        exp, n, live_map, cls, cc = _expected_list(mask, Tp)
        for what, buf, cnt, e, k in (("live", bufs[0], cnts[0], exp, n), ("cls", bufs[1], cnts[1], cls, cc)):
            assert int(cnt[0]) == k, (name, what, int(cnt[0]), k)
            assert k % 64 == 0 and k >= 192 and k <= cap
            got = buf.cpu().numpy().astype(np.uint32)
            assert np.array_equal(got[:k], e), "%s %s: list differs (first at %d)" % (name, what, int(np.nonzero(got[:k] != e)[0][0]))
            assert bool((got[k:] == 0x7FFFFFFF).all()), "%s %s: written behind the list" % (name, what)
        nl = int(live_map.sum())
        assert bool(live_map.reshape(B, L)[:, 0].all()), name + ": a [CLS] row is missing"
        assert bool((np.diff(exp[:nl].astype(np.int64)) > 0).all())
        if nl < n and not (nl == T and T == Tp):          # the padding names a row whose dY is zero: a dead row, or the first zero pad row
            assert (not live_map[exp[nl]]) if exp[nl] < T else (exp[nl] == T and T < Tp), name
        # without the [CLS] list the launch writes the live list alone
        rows = torch.full((cap + 8,), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
        count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        assert lib.mb_debug_live_rows(_lib.ptr(m), B, L, Tp, _lib.ptr(rows), _lib.ptr(count), None, None, H._stream()) == 0
        torch.cuda.synchronize()
        assert int(count[0]) == n and np.array_equal(rows.cpu().numpy().astype(np.uint32)[:n], exp), name
