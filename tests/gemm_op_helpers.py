"""Operator-level machinery for the GEMM family (csrc/gemm.hip, gemm_pp.hip, gemm_tile.h), shared by tests/test_gemm_edges_gpu.py (the
kernels, through the test hooks mb_debug_gemm_ex / mb_debug_gemm_grouped_ex / mb_debug_gemm_last_kernel) and tests/test_gemm_edges_cpu.py
(the same checks against a CPU stand-in for the kernel, with planted errors).  Nothing here needs a GPU until run_gpu() is called.

Every case is a dict of plain data (case() fills the defaults).  For a case and a dtype:
  problem()    operands exact in the compute dtype, laid out in LARGER allocations filled with NaN (guard rows behind the last row, pad
               columns behind the last column, non-natural leading dimensions), outputs filled with a canary bit pattern (a signalling
               NaN: even `+= 0` changes its bits); where the epilogue accumulates, the valid elements start from random fp32 values
  reference()  the same formula in fp64 plus, per output, the element-wise bound below
  run_gpu()    the launch -> raw output buffers and the symbol of the kernel that ran
  run_model()  the CPU stand-in: fp32 matmul, rounded to the compute dtype, written into the same layout; `plant` breaks it on purpose
  check()      canaries, finiteness, bounds; -> {output: worst |err| / bound}

Bounds (derived, not measured; S = |A| |B|^T in fp64, S' = S carried through the epilogue's linear factors: alpha, the dropout
multiplier, gelu'):
  T outputs of the linear epilogues   |err| <= u |ref| + K 2^-24 S' + tiny, u = 2^-8 (bf16: half an ulp of the one output rounding) or
                                      2^-23 (fp32); K 2^-24 S' is the worst case of ANY fp32 summation order of K exact products;
                                      tiny = 4 * 2^-24 * (|alpha acc| + |bias| + |R|): the epilogue's own fp32 operations (at most
                                      four: alpha, bias, dropout multiplier, residual / gelu'), each rounding a value no larger than
                                      the sum of its terms -- 1/64 of the bf16 term, there so that an element whose fp32 value
                                      straddles a binade does not miss the bound by a rounding of the epilogue
  fp32 outputs (both modes)           K 2^-24 S' + r 2^-24 (|init| + |ref|): r = 1 rounding of the store, or one per split-K partial sum
                                      (each atomic add rounds once; |partial| <= |init| + S is covered by the first term's S)
  column sums                         sum over rows of the accumulation terms + M 2^-24 (|init| + sum |ref|)
  EPI_BIAS_GELU's two outputs         gelu_pair is an approximation: test_ops_gpu.close() (x 1 for gelu', x 2 for gelu) is the ceiling;
                                      the worst error is reported
and in addition test_ops_gpu.close() as before, against the dtype of the OUTPUT (fp32 outputs of a bf16 launch are held to the fp32
bound); the tighter of the two holds per element."""
import ctypes as C
import re
import zlib

import numpy as np
import torch

from bert_multimodal_transformer_amd import _lib, rng

NT, NN, TN = _lib.GEMM_NT, _lib.GEMM_NN, _lib.GEMM_TN
BIAS, BIAS_GELU, BIAS_DROP_RES, ADD_RES, DGELU, ACCUM_F32, BIAS_F32 = range(7)
EPI_NAMES = ["bias", "bias_gelu", "bias_drop_res", "add_res", "dgelu", "accum_f32", "bias_f32"]
LAYOUT_NAMES = ["nt", "nn", "tn"]
F32, BF16 = _lib.DT_F32, _lib.DT_BF16
DTS = [(F32, torch.float32), (BF16, torch.bfloat16)]
MB_ERR_SHAPE, MB_ERR_MODE, MB_ERR_ARG = 1001, 1002, 1004

CANARY = {torch.float32: (torch.int32, 0x7FA5C3E1), torch.bfloat16: (torch.int16, 0x7FA5), torch.int64: (torch.int64, 0x7FA5C3E17FA5C3E1)}
GUARD = 3                    # guard rows behind every matrix
TINY = 1e-30
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01, step=3, correct_bias=1, grad_scale=0.25)


def esize(tdt):
    return 2 if tdt == torch.bfloat16 else 4


def case(name, layout, epi, M, N, nt=None, K=None, kb=128, tile=0, splits=1, pad=(8, 24, 8, 24), alpha=1.0, bias=True, R=True, drop=0.0,
         overwrite=0, cvalid=0, bseg=0, seg_gap=0, det=False, want=None, want_f32=None, rc=0, c_off=0, kguard=GUARD):
    """nt: k stages of `kb` bytes (K = nt * kb / element size: the same stage count in both dtypes) unless K is given.
    pad = extra elements of lda, ldb, ldc, ldr over the natural ones.  want / want_f32: the kernel the case is about (kernel_key())."""
    assert (nt is None) != (K is None)
    return dict(name=name, layout=layout, epi=epi, M=M, N=N, nt=nt, K=K, kb=kb, tile=tile, splits=splits, pad=tuple(pad), alpha=alpha,
                bias=bias, R=R, drop=drop, overwrite=overwrite, cvalid=cvalid, bseg=bseg, seg_gap=seg_gap, det=det, want=want,
                want_f32=want_f32, rc=rc, c_off=c_off, kguard=kguard)


def case_id(c):
    k = ("nt%d" % c["nt"]) if c["nt"] is not None else ("K%d" % c["K"])
    tags = [t for t, on in (("a%g" % c["alpha"], c["alpha"] != 1.0), ("nobias", not c["bias"]), ("noR", not c["R"]), ("drop", c["drop"] > 0),
                            ("det", c["det"]), ("ow", c["overwrite"]), ("cv%d" % c["cvalid"], c["cvalid"] > 0), ("s%d" % c["splits"], c["splits"] > 1),
                            ("seg%d" % c["bseg"], c["bseg"] > 0), ("ld+%d+%d+%d+%d" % c["pad"], c["pad"] != (8, 24, 8, 24))) if on]
    return "-".join(["%s-%s-%s-%dx%d-%s-t%d" % (c["name"], LAYOUT_NAMES[c["layout"]], EPI_NAMES[c["epi"]], c["M"], c["N"], k, c["tile"])] + tags)


def case_K(c, tdt):
    return c["K"] if c["K"] is not None else c["nt"] * c["kb"] // esize(tdt)


# ------------------------------------------------------------------------------------------------ which kernel: symbol -> key
def kernel_key(sym):
    """family:BMxBN:ring:kbytes of a GEMM kernel symbol, mangled (what the library hands out) or demangled (what a trace prints):
    g2 = gemm2_kernel (LDS-DMA ring), v1 = gemm_kernel (register-staged), pp / pn / pt = the ping-pong kernels, +ride / grouped forms."""
    s = sym.strip()
    if s.startswith("_ZN2mb"):
        j = 6
        while s[j].isdigit():
            j += 1
        n = int(s[6:j])
        fn, rest = s[j:j + n], s[j + n:]
        # the literal template arguments (L<type code><value>E) in order; type arguments (f, DF16b) carry none
        lits = [(-int(v[1:]) if v.startswith("n") else int(v)) for v in re.findall(r"L[a-z](n?[0-9]+)E", rest.split("Ev")[0] + "E")]
    else:
        s = s[5:] if s.startswith("void ") else s
        head = s.split("(")[0]
        fn = head.split("<")[0].replace("mb::", "")
        lits = []
        if "<" in head:
            for a in head[head.index("<") + 1:head.rindex(">")].split(","):
                a = a.strip()
                if a in ("true", "false"):
                    lits.append(1 if a == "true" else 0)
                elif a.lstrip("-").isdigit():
                    lits.append(int(a))
    if fn in ("gemm2_kernel", "gemm2_ride_kernel"):      # <T, BM, BN, AK, BK, MODE, NSTAGE, KB, ...>
        return "%s:%dx%d:%d:%d" % ("g2" if fn == "gemm2_kernel" else "g2ride", lits[0], lits[1], lits[5], lits[6])
    if fn == "gemm2_grouped_tn_kernel":                  # <T, BM, BN, NSTAGE, KB>
        return "g2grp:%dx%d:%d:%d" % (lits[0], lits[1], lits[2], lits[3])
    if fn == "gemm_kernel":                              # <T, BM, BN, AK, BK, MODE>: two register-staged slots of 128-byte rows
        return "v1:%dx%d:2:128" % (lits[0], lits[1])
    fixed = {"gemm_pp_kernel": "pp:256x128:3:128", "gemm_pn_kernel": "pn:128x64:3:256", "gemm_pt_kernel": "pt:256x64:3:128",
             "gemm_pn_ride_kernel": "pnride:128x64:3:256", "gemm_pt_ride_kernel": "ptride:256x64:3:128",
             "gemm_pp_grouped_tn_kernel": "ppgrp:256x128:3:128"}
    return fixed.get(fn, "?" + fn)


def last_kernel():
    buf = C.create_string_buffer(512)
    n = _lib.lib().mb_debug_gemm_last_kernel(buf, 512)
    return buf.value.decode() if n > 0 else ""


# ------------------------------------------------------------------------------------------------ which kernel: the documented selection
def _regions(M, N, bm, bn):
    tm, tn = -(-M // bm), -(-N // bn)
    best = None
    for rm in (1, 2, 4, 8):
        rn = 8 // rm
        pm, pn = -(-tm // rm), -(-tn // rn)
        cost = pm * bm + pn * bn + 4 * (pm * pn * 8 - tm * tn)
        if best is None or cost < best[0]:
            best = (cost, 8 * pm * pn)
    return best[1]


PP_SET = {(NT, BIAS), (NT, BIAS_GELU), (NN, DGELU), (TN, ACCUM_F32)}
PN_SET = {(NT, BIAS), (NT, BIAS_DROP_RES), (NT, ADD_RES), (NN, ADD_RES)}


def predict(c, tdt):
    """The kernel key (or an MB_ERR_* code) the launchers' documented selection gives this case at its defaults: include/magbert_hip.h
    (tile codes, "falls back to the next smaller one") and the comments of launch_cfg / pn_cfg / launch_tile in csrc/gemm.hip."""
    es, bf = esize(tdt), tdt == torch.bfloat16
    M, N, K, layout, epi = c["M"], c["N"], case_K(c, tdt), c["layout"], c["epi"]
    bke, epv = 128 // es, 16 // es
    lda, ldb, ldc, _ = lds_of(c, tdt)
    ak, bk = layout == TN, layout in (NN, TN)
    if N % 8 or ldc % 8:
        return MB_ERR_SHAPE
    if layout in (NT, NN) and K % bke:
        return MB_ERR_SHAPE
    if bf and ((layout == NN and N % 2) or (layout == TN and (N % 2 or M % 2))):
        return MB_ERR_SHAPE
    ok_epi = {NT: (BIAS, BIAS_F32, BIAS_GELU, BIAS_DROP_RES, ADD_RES), NN: (ADD_RES, DGELU, BIAS_F32), TN: (ACCUM_F32,)}[layout]
    if epi not in ok_epi:
        return MB_ERR_MODE

    def cfg(bm, bn):
        tiles = _regions(M, N, bm, bn)
        sp = max(1, c["splits"])
        kchunk = -(-(-(-K // sp)) // bke) * bke
        sp = -(-K // kchunk)
        v2 = K % bke == 0 and lda % epv == 0 and ldb % epv == 0 and (not ak or M % bm == 0) and (not bk or N % bn == 0)
        if c["bseg"] > 0:
            stride = seg_stride(c, tdt)
            if sp != 1 or (c["bseg"] % bn if bk else c["bseg"] % 128) or stride % epv or not v2:
                return MB_ERR_SHAPE
        if bm == 256:
            if bf and bn == 128 and v2 and sp == 1 and K // bke >= 3 and (layout, epi) in PP_SET:
                return "pp:256x128:3:128"
            return cfg(128, 128)
        if not v2:
            return "v1:%dx%d:2:128" % (bm, bn)
        ns = 2
        last = K - (sp - 1) * kchunk
        if bf and min(kchunk, last) // bke < 2:          # the two-slot bf16 loop peels two stages: a single-stage k range takes three slots
            ns = 3
        if bf and bm == 64 and bn == 64 and sp == 1 and kchunk // bke >= 2 and tiles <= 512:
            ns = 3
        return "g2:%dx%d:%d:128" % (bm, bn, ns)

    def pn(forced, tall):
        if bf:
            common = c["splits"] <= 1 and c["bseg"] <= 0 and lda % 8 == 0 and ldb % 8 == 0 and (not bk or N % 64 == 0)
            for form in (0, 1):
                if not common or (tall == 0 and form == 1) or (tall == 1 and form == 0):
                    continue
                bm, ke = (256, 64) if form else (128, 128)
                tiles = _regions(M, N, bm, 64)
                if K % ke == 0 and K // ke >= 3 and (forced or 168 <= tiles <= 256) and (not ak or M % bm == 0):
                    if (layout, epi) in PN_SET:
                        return "pt:256x64:3:128" if form else "pn:128x64:3:256"
                    break
        return cfg(64, 64)

    tile = c["tile"]
    if tile == 0:
        t128 = -(-M // 128) * -(-N // 128) * max(1, c["splits"])
        tile = 128 if t128 >= 224 else 12872
        forced = False
    else:
        forced = True
    if tile == 256:
        return cfg(256, 128) if bf else cfg(128, 128)
    if tile == 128:
        return cfg(128, 128)
    if tile == 12864:
        return cfg(128, 64)
    if forced and tile in (12872, 25672) and c["bseg"] > 0:          # a narrow ping-pong tile by name takes no segmented B
        return MB_ERR_SHAPE
    if tile == 12872:
        return pn(forced, 0 if forced else -1)
    if tile == 25672:
        return pn(forced, 1)
    return cfg(64, 64)


# ------------------------------------------------------------------------------------------------ layout
def lds_of(c, tdt):
    M, N, K, layout = c["M"], c["N"], case_K(c, tdt), c["layout"]
    pa, pb, pc, pr = c["pad"]
    nat_a = M if layout == TN else K
    nat_b = K if layout == NT else N
    if c["bseg"] > 0:
        nat_b = c["bseg"]
    return nat_a + pa, nat_b + pb, N + pc, N + pr


def seg_stride(c, tdt):
    """elements between two segments of a segmented B: one [rows][ldb] image plus the gap"""
    K, ldb = case_K(c, tdt), lds_of(c, tdt)[1]
    rows = c["N"] if c["layout"] == NT else K
    return rows * ldb + c["seg_gap"]


def canary(shape, dtype):
    it, bits = CANARY[dtype]
    return torch.full(shape, bits, dtype=it).view(dtype)


def is_canary(t):
    it, bits = CANARY[t.dtype]
    return t.contiguous().view(it) == bits


def poisoned(x, ld, guard, tdt):
    """x [r][c] (float32 values exact in tdt) inside a NaN-filled [r + guard][ld] allocation of dtype tdt"""
    r, cc = x.shape
    buf = torch.full((r + guard, ld), float("nan"), dtype=tdt)
    buf[:r, :cc] = x.to(tdt)
    return buf


def rnd(shape, seed, tdt, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 2 - 1) * scale
    return x.to(tdt).float()


def problem(c, tdt):
    """-> dict of CPU tensors: the values (A, B, bias, R, init, cs_init, mask) and the raw allocations (A_buf, B_buf, ...)"""
    M, N, K, layout, epi = c["M"], c["N"], case_K(c, tdt), c["layout"], c["epi"]
    lda, ldb, ldc, ldr = lds_of(c, tdt)
    seed = (zlib.crc32(case_id(c).encode()) & 0xFFFF) * 16
    p = dict(K=K, lda=lda, ldb=ldb, ldc=ldc, ldr=ldr)
    A = rnd((K, M) if layout == TN else (M, K), seed + 1, tdt)
    B = rnd((N, K) if layout == NT else (K, N), seed + 2, tdt, 0.1)          # asymmetric operands: a transposed C-write cannot pass
    p["A"], p["B"] = A, B
    kg = c["kguard"]
    p["A_buf"] = poisoned(A, lda, kg if layout == TN else GUARD, tdt)
    if c["bseg"] > 0:
        seg, stride = c["bseg"], seg_stride(c, tdt)
        nseg = (K if layout == NT else N) // seg
        flat = torch.full((nseg * stride + GUARD * ldb,), float("nan"), dtype=tdt)
        for s in range(nseg):
            piece = B[:, s * seg:(s + 1) * seg]
            flat[s * stride:s * stride + piece.shape[0] * ldb].view(piece.shape[0], ldb)[:, :seg] = piece.to(tdt)
        p["B_buf"] = flat
    else:
        p["B_buf"] = poisoned(B, ldb, kg if layout != NT else GUARD, tdt)
    if c["bias"] and epi in (BIAS, BIAS_GELU, BIAS_DROP_RES, BIAS_F32):
        p["bias"] = rnd((N,), seed + 3, torch.float32)
        p["bias_buf"] = torch.cat([p["bias"], torch.full((8,), float("nan"))])
    if c["R"] and epi in (BIAS_DROP_RES, ADD_RES, DGELU):
        p["R"] = rnd((M, N), seed + 4, tdt)
        p["R_buf"] = poisoned(p["R"], ldr, GUARD, tdt)
    if c["drop"] > 0:
        p["key"] = (11, 3, 17, c["drop"])
        p["mask"] = torch.from_numpy(rng.keep_mult(M * N, rng.make_key(*p["key"]))).view(M, N).double()
    # outputs: canaries everywhere; accumulating epilogues start from random fp32 values on what they own
    if epi in (ACCUM_F32, BIAS_F32):
        off = c["c_off"]                                  # the output starts `off` floats into its allocation (a 4-byte-aligned base)
        buf = canary((off + (M + GUARD) * ldc,), torch.float32)
        if epi == ACCUM_F32 and not c["overwrite"]:
            cols = c["cvalid"] if c["cvalid"] > 0 else N
            p["init"] = rnd((M, cols), seed + 5, torch.float32)
            buf[off:off + M * ldc].view(M, ldc)[:, :cols] = p["init"]
        p["Cf_buf"] = buf
    else:
        p["C_buf"] = canary((M + GUARD, ldc), tdt)
        if epi == BIAS_GELU:
            p["C2_buf"] = canary((M + GUARD, ldc), tdt)
        if epi == DGELU:
            p["cs_init"] = rnd((N,), seed + 6, torch.float32)
            p["cs_buf"] = torch.cat([p["cs_init"], canary((8,), torch.float32)])
            if c["det"]:
                p["sh_buf"] = torch.cat([torch.zeros(N, dtype=torch.int64), canary((8,), torch.int64)])
    return p


# ------------------------------------------------------------------------------------------------ fp64 reference and bounds
def reference(c, tdt, p):
    """-> {output name: (ref fp64, bound fp64, close-dtype, close-scale)}; output names: C, C2, Cf, colsum"""
    M, N, K, layout, epi = c["M"], c["N"], p["K"], c["layout"], c["epi"]
    A, B = p["A"].double(), p["B"].double()
    if layout == TN:
        acc, S = A.t() @ B, A.abs().t() @ B.abs()
    elif layout == NN:
        acc, S = A @ B, A.abs() @ B.abs()
    else:
        acc, S = A @ B.t(), A.abs() @ B.abs().t()
    u = 2.0 ** -8 if tdt == torch.bfloat16 else 2.0 ** -23
    dt = BF16 if tdt == torch.bfloat16 else F32
    e32 = 2.0 ** -24
    bias = p["bias"].double() if "bias" in p else torch.zeros(N, dtype=torch.float64)
    R = p["R"].double() if "R" in p else torch.zeros(M, N, dtype=torch.float64)
    mask = p.get("mask", torch.ones(M, N, dtype=torch.float64))
    alpha = float(np.float32(c["alpha"]))
    out = {}

    def tiny(*terms):
        return 4 * e32 * sum(t.abs() for t in terms) + TINY

    if epi == BIAS or epi == BIAS_F32:
        ref, Sp = alpha * acc + bias, abs(alpha) * S
        if epi == BIAS:
            out["C"] = (ref, u * ref.abs() + K * e32 * Sp + tiny(alpha * acc, bias.expand_as(acc)), dt, 1.0)
        else:
            out["Cf"] = (ref, K * e32 * Sp + e32 * ref.abs() + tiny(alpha * acc, bias.expand_as(acc)), F32, 1.0)
    elif epi == BIAS_GELU:
        uu = acc + bias
        d = 0.5 * (1 + torch.erf(uu / 2 ** 0.5)) + uu * torch.exp(-0.5 * uu * uu) / (2 * np.pi) ** 0.5
        g = uu * 0.5 * (1 + torch.erf(uu / 2 ** 0.5))
        out["C"] = (d, None, dt, 1.0)
        out["C2"] = (g * mask, None, dt, 2.0)
    elif epi == BIAS_DROP_RES:
        ref = (acc + bias) * mask + R
        out["C"] = (ref, u * ref.abs() + K * e32 * S * mask + tiny((acc + bias) * mask, R), dt, 1.0)
    elif epi == ADD_RES:
        ref = acc + R
        out["C"] = (ref, u * ref.abs() + K * e32 * S + tiny(acc, R), dt, 1.0)
    elif epi == DGELU:
        ref, Sp = acc * R * mask, S * R.abs() * mask
        out["C"] = (ref, u * ref.abs() + K * e32 * Sp + tiny(ref), dt, 1.0)
        cs0 = p["cs_init"].double()
        out["colsum"] = (cs0 + ref.sum(0), (K * e32 * Sp).sum(0) + M * e32 * (cs0.abs() + ref.abs().sum(0)) + TINY, dt, 1.0)
    elif epi == ACCUM_F32:
        cols = c["cvalid"] if c["cvalid"] > 0 else N
        init = p["init"].double() if "init" in p else torch.zeros(M, cols, dtype=torch.float64)
        ref = init + acc[:, :cols]
        kchunk = -(-(-(-K // max(1, c["splits"]))) // (128 // esize(tdt))) * (128 // esize(tdt))
        r = -(-K // kchunk)
        out["Cf"] = (ref, K * e32 * S[:, :cols] + r * e32 * (init.abs() + ref.abs()) + TINY, F32, 1.0)
    return out


def close_tol(dt, ref, scale=1.0):
    """test_ops_gpu.tol(): the global bound every GEMM result has been held to so far"""
    s = float(ref.abs().max())
    return ((2e-5 * s + 1e-6) if dt == F32 else (1.2e-2 * s + 1e-6)) * scale


# ------------------------------------------------------------------------------------------------ the outputs of a run
def valid_view(c, name, buf, p):
    """-> (the [M][cols] valid region as float64, a bool map of the same shape as `buf` that is True on what the kernel owns)"""
    M, N, ldc = c["M"], c["N"], p["ldc"]
    own = torch.zeros(buf.shape, dtype=torch.bool)
    if name == "colsum":
        own[:N] = True
        return buf[:N].double(), own
    if name == "Cf":
        off = c["c_off"]
        cols = c["cvalid"] if (c["cvalid"] > 0 and c["epi"] == ACCUM_F32) else N
        v = buf[off:off + M * ldc].view(M, ldc)[:, :cols]
        own[off:off + M * ldc].view(M, ldc)[:, :cols] = True
        return v.double(), own
    own[:M, :N] = True
    return buf[:M, :N].double(), own


def check(c, tdt, p, outs, ref=None, what=""):
    """outs: {name: raw buffer}.  Canaries, finiteness, element-wise bound, close().  -> {name: (worst |err| / bound, max |err|)}"""
    ref = ref if ref is not None else reference(c, tdt, p)
    res = {}
    for name, (r, bound, cdt, scale) in ref.items():
        buf = outs[name]
        got, own = valid_view(c, name, buf, p)
        intact = is_canary(buf)
        assert bool(intact[~own].all()), "%s %s: %d element(s) outside the output were written (first at flat index %d)" % (
            what, name, int((~intact[~own]).sum()), int((~intact & ~own).flatten().nonzero()[0]))
        assert bool(torch.isfinite(got).all()), "%s %s: %d non-finite element(s) in the output" % (what, name, int((~torch.isfinite(got)).sum()))
        err = (got - r).abs()
        ceil = close_tol(cdt, r, scale)
        lim = torch.full_like(err, ceil) if bound is None else torch.minimum(bound, torch.full_like(err, ceil))
        ratio = err / lim
        worst = int(ratio.argmax())
        res[name] = (float(ratio.flatten()[worst]), float(err.max()))
        assert float(ratio.flatten()[worst]) <= 1.0, "%s %s: |err| %.3e > bound %.3e at element %s (ref %.6e), %d element(s) over" % (
            what, name, float(err.flatten()[worst]), float(lim.flatten()[worst]), tuple(int(i) for i in np.unravel_index(worst, tuple(err.shape))),
            float(r.flatten()[worst]), int((ratio > 1.0).sum()))
    if "sh_buf" in p and "shadow" in outs:                # deterministic column sums: the fold leaves zeros and the canary behind
        sh = outs["shadow"]
        assert bool((sh[:c["N"]] == 0).all()) and bool(is_canary(sh)[c["N"]:].all()), what + " colsum shadow"
    return res


# ------------------------------------------------------------------------------------------------ the CPU stand-in for the kernel
def gather_B(c, tdt, p, plant=None):
    """B's values as the kernel reads them: from the raw allocation, by the addressing rule of GemmArgs"""
    K, N, layout, ldb = p["K"], c["N"], c["layout"], p["ldb"]
    rows, cols = (N, K) if layout == NT else (K, N)
    flat = p["B_buf"].flatten()
    if c["bseg"] <= 0:
        return flat[:rows * ldb].view(rows, ldb)[:, :cols].float()
    seg, stride = c["bseg"], seg_stride(c, tdt)
    parts = []
    for s in range(cols // seg):
        st = s * seg if (plant == "seg_natural" and s == 1) else s * stride       # planted: segment 1 found at the natural stride
        parts.append(flat[st:st + rows * ldb].view(rows, ldb)[:, :seg].float())
    return torch.cat(parts, 1)


def run_model(c, tdt, p, plant=None, tile=(64, 64)):
    """fp32 matmul + the epilogue in fp32, rounded to the compute dtype, stored into copies of the poisoned outputs.  plant:
    drop_k_row | last_row_above | shift_tile_cols | store_col_N | store_row_M | seg_natural"""
    M, N, K, layout, epi, ldc = c["M"], c["N"], p["K"], c["layout"], c["epi"], p["ldc"]
    rows_a = K if layout == TN else M
    A = p["A_buf"][:rows_a, :(M if layout == TN else K)].float()
    B = gather_B(c, tdt, p, plant)
    A2 = A.t() if layout == TN else A
    B2 = B if layout != NT else B.t()
    acc = A2 @ B2
    if plant == "drop_k_row":                             # one k element left out, in one row only
        r = M - 1
        acc[r] = acc[r] - A2[r, K // 2] * B2[K // 2]
    if plant == "last_row_above":                         # the last row of a ragged tile computed from the row above
        acc[M - 1] = acc[M - 2]
    alpha = np.float32(c["alpha"])
    bias = p["bias"] if "bias" in p else torch.zeros(N)
    R = p["R"] if "R" in p else torch.zeros(M, N)
    mask = p["mask"].float() if "mask" in p else torch.ones(M, N)
    outs = {}

    def store_T(name, v):
        v = v.clone()
        if plant == "shift_tile_cols":                    # the first tile's columns, rotated by 8
            v[:tile[0], :tile[1]] = torch.roll(v[:tile[0], :tile[1]], 8, 1)
        buf = p[name + "_buf"].clone()
        buf[:M, :N] = v.to(tdt)
        if plant == "store_col_N":
            buf[M // 2, N] = 0.0
        if plant == "store_row_M":
            buf[M, 0] = 0.0
        outs[name] = buf

    if epi == BIAS:
        store_T("C", acc * alpha + bias)
    elif epi == BIAS_GELU:
        uu = (acc + bias).double()
        store_T("C", (0.5 * (1 + torch.erf(uu / 2 ** 0.5)) + uu * torch.exp(-0.5 * uu * uu) / (2 * np.pi) ** 0.5).float())
        store_T("C2", torch.nn.functional.gelu(uu.float()) * mask)
    elif epi == BIAS_DROP_RES:
        store_T("C", (acc + bias) * mask + R)
    elif epi == ADD_RES:
        store_T("C", acc + R)
    elif epi == DGELU:
        v = acc * (R * mask)
        store_T("C", v)
        cs = p["cs_buf"].clone()
        cs[:N] = cs[:N] + v.sum(0)
        outs["colsum"] = cs
        if "sh_buf" in p:
            outs["shadow"] = p["sh_buf"].clone()
    else:
        off = c["c_off"]
        buf = p["Cf_buf"].clone()
        cols = c["cvalid"] if (c["cvalid"] > 0 and epi == ACCUM_F32) else N
        view = buf[off:off + M * ldc].view(M, ldc)
        v = (acc * alpha + bias) if epi == BIAS_F32 else acc
        if plant == "shift_tile_cols":
            v = v.clone()
            v[:tile[0], :tile[1]] = torch.roll(v[:tile[0], :tile[1]], 8, 1)
        view[:, :cols] = (v[:, :cols] + p["init"]) if "init" in p else v[:, :cols]
        if plant == "store_col_N":
            view[M // 2, cols] = 0.0
        if plant == "store_row_M":
            buf[off + M * ldc] = 0.0
        outs["Cf"] = buf
    return outs


# ------------------------------------------------------------------------------------------------ the GPU run
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ride_args(ride):
    """ride: None or dict(p, g, m, v, shadow (or None), n4, blocks, zero_grad, adam_dev) of device tensors"""
    if ride is None:
        return [None, None, None, None, None, 0, 0, 0] + _adam_scalars() + [None]
    return [_lib.ptr(ride["p"]), _lib.ptr(ride["g"]), _lib.ptr(ride["m"]), _lib.ptr(ride["v"]), _lib.ptr(ride["shadow"]), ride["n4"],
            ride["blocks"], ride["zero_grad"]] + _adam_scalars() + [_lib.ptr(ride["adam_dev"])]


def _adam_scalars():
    a = ADAM
    return [a["lr"], a["beta1"], a["beta2"], a["eps"], a["weight_decay"], a["step"], a["correct_bias"], a["grad_scale"]]


def run_gpu(c, dt, tdt, p, dev="cuda:0", ride=None):
    """one mb_debug_gemm_ex launch of the case -> (rc, {name: raw output buffer on the CPU}, kernel symbol, rider tile count)"""
    L = _lib.lib()
    d = {k: v.to(dev) for k, v in p.items() if k.endswith("_buf")}
    M, N, K, epi = c["M"], c["N"], p["K"], c["epi"]
    key = _lib.make_dropkey(*p["key"]) if "key" in p else None
    Cf = d.get("Cf_buf")
    cf_ptr = None
    if Cf is not None:
        cf_ptr = C.c_void_p(Cf.data_ptr() + 4 * c["c_off"])
    elif "cs_buf" in d:
        cf_ptr = _lib.ptr(d["cs_buf"])
    tiles = C.c_int(0)
    stride = seg_stride(c, tdt) if c["bseg"] > 0 else 0
    rc = L.mb_debug_gemm_ex(dt, c["layout"], epi, M, N, K, _lib.ptr(d["A_buf"]), p["lda"], _lib.ptr(d["B_buf"]), p["ldb"],
                            _lib.ptr(d.get("C_buf")), p["ldc"], _lib.ptr(d.get("C2_buf")), cf_ptr, _lib.ptr(d.get("bias_buf")),
                            _lib.ptr(d.get("R_buf")), p["ldr"], c["alpha"], C.byref(key) if key is not None else None, c["splits"],
                            c["tile"], c["bseg"], stride, c["cvalid"], c["overwrite"], _lib.ptr(d.get("sh_buf")), 1 if c["det"] else 0,
                            *_ride_args(ride), C.byref(tiles), _stream())
    torch.cuda.synchronize()
    outs = {}
    for name, k in (("C", "C_buf"), ("C2", "C2_buf"), ("Cf", "Cf_buf"), ("colsum", "cs_buf"), ("shadow", "sh_buf")):
        if k in d:
            outs[name] = d[k].cpu()
    return rc, outs, (last_kernel() if rc == 0 else ""), tiles.value


# ------------------------------------------------------------------------------------------------ grouped weight gradients with cvalid
SPARE = 3                    # columns of the shared output tensors that no problem owns


def grouped_problem(tdt, K, H=128, V=47, A=74, Vp=64, overwrite=0):
    """MAG's six weight-gradient problems (engine_common.h mag_bwd_impl): (text | visual | acoustic operand) x (gate half | projection half
    of the dZ columns), stored dword-wise into column ranges of dW_hv [H][V + H], dW_ha [H][A + H], dW_v [H][V], dW_a [H][A] -- here each
    SPARE columns wider, so that there are columns nobody owns.  The padded operand columns [V, Vp) hold random values, not zeros: what
    a cvalid overrun would add is visible with `+=` as well."""
    g = dict(K=K, H=H, overwrite=overwrite, tdt=tdt, off=1, outs=["hv", "ha", "v", "a"])
    ops = {"dZe": (2 * H, 1), "dZv": (2 * H, 2), "dZa": (2 * H, 3), "text": (H, 4), "vp": (Vp, 5), "ap": (Vp if A <= Vp else 2 * Vp, 6)}
    Ap = ops["ap"][0]
    for name, (cols, sd) in ops.items():
        g[name] = rnd((K, cols), 100 + sd, tdt, 0.1 if name in ("text", "vp", "ap") else 1.0)
        g[name + "_buf"] = poisoned(g[name], cols + 8, GUARD, tdt)
    widths = {"hv": V + H + SPARE, "ha": A + H + SPARE, "v": V + SPARE, "a": A + SPARE}
    for name, wd in widths.items():
        buf = canary((1 + (H + GUARD) * wd,), torch.float32)       # the tensor starts one float into its allocation
        g["W" + name + "_ld"] = wd
        g["W" + name + "_buf"] = buf
    # (M, N, dY, dY column offset, X, output tensor, output column offset, cvalid)
    g["probs"] = [(H, H, "dZe", 0, "text", "hv", V, H), (H, H, "dZe", H, "text", "ha", A, H),
                  (H, Vp, "dZv", 0, "vp", "hv", 0, V), (H, Vp, "dZv", H, "vp", "v", 0, V),
                  (H, Ap, "dZa", 0, "ap", "ha", 0, A), (H, Ap, "dZa", H, "ap", "a", 0, A)]
    if not overwrite:
        for i, (M, N, dy, yo, x, out, co, cv) in enumerate(g["probs"]):
            init = rnd((M, cv), 200 + i, torch.float32)
            g["init%d" % i] = init
            wd = g["W" + out + "_ld"]
            g["W" + out + "_buf"][1:1 + M * wd].view(M, wd)[:, co:co + cv] = init
    return g


def grouped_plain(tdt, K, shapes, overwrite=0):
    """independent whole-tile problems dW_i [M_i][N_i] (+)= dY_i^T X_i with aligned outputs N_i + 8 floats wide: the rider hosts"""
    g = dict(K=K, H=None, overwrite=overwrite, tdt=tdt, off=0, outs=[], probs=[])
    for i, (M, N) in enumerate(shapes):
        for name, cols, sc in (("dY%d" % i, M, 1.0), ("X%d" % i, N, 0.1)):
            g[name] = rnd((K, cols), 300 + 2 * i + (name[0] == "X"), tdt, sc)
            g[name + "_buf"] = poisoned(g[name], cols + 8, GUARD, tdt)
        o = "o%d" % i
        g["outs"].append(o)
        g["W" + o + "_ld"] = N + 8
        g["W" + o + "_buf"] = canary(((M + GUARD) * (N + 8),), torch.float32)
        g["probs"].append((M, N, "dY%d" % i, 0, "X%d" % i, o, 0, N))
        if not overwrite:
            g["init%d" % i] = rnd((M, N), 400 + i, torch.float32)
            g["W" + o + "_buf"][:M * (N + 8)].view(M, N + 8)[:, :N] = g["init%d" % i]
    return g


def grouped_reference(g):
    """-> per output tensor: (ref [H][ld] fp64, bound, owned bool map) over the [H][ld] image"""
    K, tdt = g["K"], g["tdt"]
    e32 = 2.0 ** -24
    out = {}
    for i, (M, N, dy, yo, x, o, co, cv) in enumerate(g["probs"]):
        wd = g["W" + o + "_ld"]
        if o not in out:
            out[o] = [torch.zeros(M, wd, dtype=torch.float64), torch.zeros(M, wd, dtype=torch.float64), torch.zeros(M, wd, dtype=torch.bool)]
        Y, X = g[dy][:, yo:yo + M].double(), g[x][:, :cv].double()
        init = g["init%d" % i].double() if ("init%d" % i) in g else torch.zeros(M, cv, dtype=torch.float64)
        ref = init + Y.t() @ X
        S = Y.abs().t() @ X.abs()
        assert not bool(out[o][2][:, co:co + cv].any())
        out[o][0][:, co:co + cv] = ref
        out[o][1][:, co:co + cv] = K * e32 * S + e32 * (init.abs() + ref.abs()) + TINY
        out[o][2][:, co:co + cv] = True
    return out


def grouped_check(g, outs, ref=None, what=""):
    ref = ref if ref is not None else grouped_reference(g)
    off, res = g["off"], {}
    for o, (r, bound, own) in ref.items():
        wd, buf, H = g["W" + o + "_ld"], outs[o], r.shape[0]
        img = buf[off:off + H * wd].view(H, wd)
        intact = is_canary(buf)
        own_flat = torch.zeros(buf.shape, dtype=torch.bool)
        own_flat[off:off + H * wd] = own.flatten()
        assert bool(intact[~own_flat].all()), "%s dW_%s: %d element(s) no problem owns were written (first at flat index %d)" % (
            what, o, int((~intact[~own_flat]).sum()), int((~intact & ~own_flat).nonzero()[0]))
        got = img.double()[own]
        assert bool(torch.isfinite(got).all()), "%s dW_%s: non-finite output" % (what, o)
        err = (got - r[own]).abs()
        lim = torch.minimum(bound[own], torch.full_like(err, close_tol(F32, r[own])))
        ratio = err / lim
        res[o] = (float(ratio.max()), float(err.max()))
        assert float(ratio.max()) <= 1.0, "%s dW_%s: |err| / bound %.3f (max |err| %.3e), %d element(s) over" % (
            what, o, float(ratio.max()), float(err.max()), int((ratio > 1).sum()))
    return res


def grouped_model(g, plant=None):
    outs = {}
    for o in g["outs"]:
        outs[o] = g["W" + o + "_buf"].clone()
    off = g["off"]
    for i, (M, N, dy, yo, x, o, co, cv) in enumerate(g["probs"]):
        wd, H = g["W" + o + "_ld"], M
        Y = g[dy + "_buf"][:g["K"], yo:yo + M].float()
        X = g[x + "_buf"][:g["K"], :N].float()
        acc = Y.t() @ X
        img = outs[o][off:off + H * wd].view(H, wd)
        keep = cv + 1 if (plant == "cvalid_overrun" and i == 3) else cv            # planted: one column past cvalid is stored
        if ("init%d" % i) in g:
            tgt = img[:, co:co + keep].clone()
            tgt.view(torch.int32)[is_canary(tgt)] = 0                             # (`+=` onto what is there; a canary is not a number)
            img[:, co:co + keep] = tgt + acc[:, :keep]
        else:
            img[:, co:co + keep] = acc[:, :keep]
    return outs


def _ptr_arr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _int_arr(v):
    return (C.c_int * len(v))(*v)


def grouped_run_gpu(dt, g, tile, stages, dev="cuda:0", ride=None, probs=None, cvalid=None):
    """one mb_debug_gemm_grouped_ex launch -> (rc, {tensor: raw buffer}, kernel symbol)"""
    L = _lib.lib()
    es = esize(g["tdt"])
    d = {k: v.to(dev) for k, v in g.items() if k.endswith("_buf")}
    probs = probs if probs is not None else g["probs"]
    n = len(probs)
    Ms, Ns = [p[0] for p in probs], [p[1] for p in probs]
    dY = [d[p[2] + "_buf"].data_ptr() + p[3] * es for p in probs]
    ldy = [d[p[2] + "_buf"].shape[1] for p in probs]
    X = [d[p[4] + "_buf"].data_ptr() for p in probs]
    ldx = [d[p[4] + "_buf"].shape[1] for p in probs]
    dW = [d["W" + p[5] + "_buf"].data_ptr() + 4 * (g["off"] + p[6]) for p in probs]
    ldw = [g["W" + p[5] + "_ld"] for p in probs]
    cv = cvalid if cvalid is not None else [p[7] for p in probs]
    rc = L.mb_debug_gemm_grouped_ex(dt, n, _int_arr(Ms), _int_arr(Ns), g["K"], _ptr_arr(dY), _int_arr(ldy), _ptr_arr(X), _int_arr(ldx),
                                    _ptr_arr(dW), _int_arr(ldw), _int_arr(cv), _int_arr([g["overwrite"]] * n), tile, stages,
                                    *_ride_args(ride), _stream())
    torch.cuda.synchronize()
    return rc, {o: d["W" + o + "_buf"].cpu() for o in g["outs"]}, (last_kernel() if rc == 0 else "")


# ------------------------------------------------------------------------------------------------ riders
RIDE_TAIL = 64               # canary floats behind the 4 * n4 a rider owns


def ride_state(n4, blocks, zero_grad, shadow, dev="cuda:0", seed=7):
    """device tensors of one rider: p / g / m / v of 4 * n4 floats (+ a canary tail), the bf16 shadow (or None), the AdamArgs buffer"""
    n = 4 * n4
    gen = torch.Generator().manual_seed(seed)
    st = dict(n4=n4, blocks=blocks, zero_grad=zero_grad)
    for name, f in (("p", lambda: torch.randn(n, generator=gen)), ("g", lambda: torch.randn(n, generator=gen) * 0.1),
                    ("m", lambda: torch.randn(n, generator=gen) * 0.01), ("v", lambda: torch.rand(n, generator=gen) * 1e-3)):
        st[name] = torch.cat([f(), canary((RIDE_TAIL,), torch.float32)]).to(dev)
    st["shadow"] = canary((n + RIDE_TAIL,), torch.bfloat16).to(dev) if shadow else None
    st["adam_dev"] = torch.zeros(8, dtype=torch.float32, device=dev)
    return st


def ride_clone(st):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}


def ride_expected(st):
    """what mb_adamw_step makes of copies of the same buffers: every parameter decays, the whole range is shadowed (adamw_dev.h)"""
    e = ride_clone(st)
    n = 4 * st["n4"]
    a = ADAM
    _lib.check(_lib.lib().mb_adamw_step(_lib.ptr(e["p"]), _lib.ptr(e["g"]), _lib.ptr(e["m"]), _lib.ptr(e["v"]), _lib.ptr(e["shadow"]), n, n, 0,
                                        n if e["shadow"] is not None else 0, a["lr"], a["beta1"], a["beta2"], a["eps"], a["weight_decay"],
                                        a["step"], a["correct_bias"], a["grad_scale"], st["zero_grad"], _stream()))
    torch.cuda.synchronize()
    return e


def ride_check(got, exp, what=""):
    """same bits as the stand-alone update on [0, 4 * n4), canaries behind"""
    for k in ("p", "g", "m", "v", "shadow"):
        if got[k] is None:
            continue
        it = CANARY[got[k].dtype][0]
        a, b = got[k].cpu().view(it), exp[k].cpu().view(it)
        assert torch.equal(a, b), "%s rider %s: %d element(s) differ from mb_adamw_step's bits (first at %d)" % (
            what, k, int((a != b).sum()), int((a != b).nonzero()[0]))
        assert bool(is_canary(got[k].cpu())[4 * got["n4"]:].all()), "%s rider %s: written behind 4 * n4" % (what, k)


# ------------------------------------------------------------------------------------------------ the case lists (plain data)
NT_EPIS = [BIAS, BIAS_GELU, BIAS_DROP_RES, ADD_RES, BIAS_F32]
NN_EPIS = [ADD_RES, DGELU, BIAS_F32]
# family: tile code, tile rows / columns, stage counts from the loop's minimum up, bytes of k per stage, the (layout, epilogue) pairs the
# family's kernel is instantiated for (what is not in the list is a documented fallback: FALLBACK_CASES), the bf16 kernel it means
FAMILIES = {
    # 64 x 64: three ring slots up to 512 padded tiles (plain loop: any stage count, 1 included)
    "r64": dict(tile=64, bm=64, bn=64, nts=[1, 2, 3, 4, 7], kb=128, want="g2:64x64:3:128",
                pairs=[(NT, e) for e in NT_EPIS] + [(NN, e) for e in NN_EPIS] + [(TN, ACCUM_F32)]),
    # 128 x 128 two slots: pipelined loop with two peeled stages; a single stage goes to three slots
    "t128": dict(tile=128, bm=128, bn=128, nts=[1, 2, 3, 4, 5], kb=128, want="g2:128x128:",
                 pairs=[(NT, e) for e in NT_EPIS] + [(NN, e) for e in NN_EPIS] + [(TN, ACCUM_F32)]),
    # 128 x 64 four waves (tile code 12864)
    "w12864": dict(tile=12864, bm=128, bn=64, nts=[2, 3], kb=128, want="g2:128x64:2:128",
                   pairs=[(NT, BIAS), (NT, BIAS_DROP_RES), (NN, ADD_RES), (NN, DGELU), (TN, ACCUM_F32)]),
    # 256 x 128 eight-wave ping-pong: three slots, three peeled stages
    "pp256": dict(tile=256, bm=256, bn=128, nts=[3, 4, 5, 6, 7], kb=128, want="pp:256x128:3:128",
                  pairs=[(NT, BIAS), (NT, BIAS_GELU), (NN, DGELU), (TN, ACCUM_F32)]),
    # 128 x 64 ping-pong, 256 bytes (128 k) per stage
    "pn": dict(tile=12872, bm=128, bn=64, nts=[3, 4, 5, 6, 7], kb=256, want="pn:128x64:3:256",
               pairs=[(NT, BIAS), (NT, BIAS_DROP_RES), (NT, ADD_RES), (NN, ADD_RES)]),
    # 256 x 64 ping-pong, 128 bytes (64 k) per stage
    "pt": dict(tile=25672, bm=256, bn=64, nts=[3, 4, 5, 6, 7], kb=128, want="pt:256x64:3:128",
               pairs=[(NT, BIAS), (NT, BIAS_DROP_RES), (NT, ADD_RES), (NN, ADD_RES)]),
}
SEAM_M = [1, 127, 128, 129, 255, 257]          # the 128-row seam between the two wave groups of the 256-row tiles


def _epi_kw(epi, i):
    """the riders of an epilogue, varied with the case index: alpha != 1, a dropout key, deterministic column sums"""
    kw = {}
    if epi in (BIAS, BIAS_F32):
        kw["alpha"] = (0.5, 0.37, 1.0)[i % 3]
    if epi == BIAS_DROP_RES or (epi in (BIAS_GELU, DGELU) and i % 2 == 0):
        kw["drop"] = 0.1
    if epi == DGELU and i % 3 == 1:
        kw["det"] = True
    return kw


def family_cases(fam):
    f = FAMILIES[fam]
    bm, bn, tile, kb = f["bm"], f["bn"], f["tile"], f["kb"]
    out, i = [], 0

    def add(layout, epi, M, N, nt, **kw):
        nonlocal i
        k = _epi_kw(epi, i)
        k.update(kw)
        out.append(case(fam, layout, epi, M, N, nt=nt, kb=kb, tile=tile, want=f["want"], **k))
        i += 1

    # 1. every stage count of the loop, for every (layout, epilogue) the kernel exists for, at a ragged shape with more than one tile
    for nt in f["nts"]:
        for layout, epi in f["pairs"]:
            if layout == NT:
                add(layout, epi, bm + 1, 200, nt)
            elif layout == NN:
                add(layout, epi, bm + 1, 2 * bn, nt)           # (a k-major operand needs whole tiles, else the v1 kernel runs: V1_CASES)
            else:
                add(layout, epi, 2 * bm, bn, nt)
    # 2. row and column edges at the second-smallest stage count: M one below, at and one above a tile; N one tile, tile + 8, 200
    nt = f["nts"][1]
    edges_m = [bm - 1, bm, bm + 1] + (SEAM_M if bm == 256 else [])
    nt_pairs = [p for p in f["pairs"] if p[0] == NT]
    nn_pairs = [p for p in f["pairs"] if p[0] == NN]
    for j, M in enumerate(edges_m):
        for q, N in enumerate([bn, bn + 8, 200]):
            layout, epi = nt_pairs[(j + q) % len(nt_pairs)]
            add(layout, epi, M, N, nt)
        layout, epi = nn_pairs[j % len(nn_pairs)]
        add(layout, epi, M, bn, nt)
    # 3. one natural-stride case
    layout, epi = f["pairs"][0]
    add(layout, epi, bm + 1, 200, nt, pad=(0, 0, 0, 0))
    return out


def p64_cases():
    """the 64 x 64 two-slot pipelined loop (bf16): more than 512 padded tiles -- 23 x 24 -- with K at the loop's minimum and just above"""
    out = []
    for i, nt in enumerate([2, 3, 4, 5]):
        layout, epi = [(NT, BIAS), (NN, ADD_RES), (NT, BIAS_DROP_RES), (NN, DGELU)][i]
        out.append(case("p64", layout, epi, 23 * 64 - 7, 24 * 64, nt=nt, tile=64, want="g2:64x64:2:128", **_epi_kw(epi, i)))
    out.append(case("p64", TN, ACCUM_F32, 23 * 64, 24 * 64, nt=2, tile=64, want="g2:64x64:2:128"))
    return out


def epilogue_cases():
    """what the family sweeps do not vary: bias = NULL, R = NULL, overwrite against +=, alpha with the fp32 output, on the 64 x 64 and the
    128 x 128 kernels at a ragged edge"""
    out = []
    for tile, bm, want in ((64, 64, "g2:64x64:3:128"), (128, 128, "g2:128x128:2:128")):
        kw = dict(nt=2, tile=tile, want=want)
        out += [case("epi", NT, BIAS, bm + 1, 200, bias=False, alpha=0.37, **kw),
                case("epi", NT, BIAS_F32, bm + 1, 200, alpha=0.37, **kw),
                case("epi", NT, BIAS_F32, bm + 1, 200, bias=False, **kw),
                case("epi", NT, BIAS_GELU, bm + 1, 200, bias=False, drop=0.1, **kw),
                case("epi", NT, BIAS_DROP_RES, bm + 1, 200, R=False, drop=0.1, **kw),
                case("epi", NT, ADD_RES, bm + 1, 200, R=False, **kw),
                case("epi", NN, ADD_RES, bm + 1, 2 * tile, R=False, **kw),
                case("epi", NN, DGELU, bm + 1, 2 * tile, drop=0.1, det=True, **kw),
                case("epi", NN, DGELU, bm - 1, 2 * tile, drop=0.1, **kw),
                case("epi", NN, BIAS_F32, bm + 1, 2 * tile, alpha=0.37, **kw),
                case("epi", TN, ACCUM_F32, 2 * tile, tile, overwrite=1, **kw),
                case("epi", TN, ACCUM_F32, 2 * tile, tile, overwrite=0, **kw),
                # cvalid: dword stores of the first 47 columns only, from a base that is 4-byte aligned and no more
                case("epi", TN, ACCUM_F32, 2 * tile, tile, overwrite=1, cvalid=47, c_off=1, **kw),
                case("epi", TN, ACCUM_F32, 2 * tile, tile, overwrite=0, cvalid=47, c_off=1, **kw)]
    return out


def v1_cases():
    """the register-staged v1 kernel: what the LDS-DMA kernels refuse"""
    out = []
    for tile in (64, 128):
        w = "v1:%dx%d:2:128" % (tile, tile)
        out += [case("v1", NN, ADD_RES, tile + 1, 200, nt=2, tile=tile, want=w, want_f32=w),            # k-major B, ragged N
                case("v1", NN, DGELU, tile - 1, 200, nt=3, tile=tile, drop=0.1, want=w, want_f32=w),
                case("v1", TN, ACCUM_F32, tile + 36, tile, nt=2, tile=tile, want=w, want_f32=w),        # k-major A, ragged M
                case("v1", TN, ACCUM_F32, tile, tile + 8, K=150, tile=tile, want=w, want_f32=w),        # K is no whole stage
                case("v1", TN, ACCUM_F32, tile, tile, K=150, tile=tile, splits=2, want=w, want_f32=w),
                # a leading dimension that is no 16-byte multiple (A, then B)
                case("v1", NT, BIAS, tile + 1, 72, nt=2, tile=tile, pad=(2, 24, 8, 24), want=w, want_f32=w),
                case("v1", NT, BIAS_DROP_RES, tile + 1, 72, nt=2, tile=tile, pad=(8, 2, 8, 24), drop=0.1, want=w, want_f32=w),
                case("v1", NN, ADD_RES, tile + 1, tile, nt=2, tile=tile, pad=(8, 2, 8, 24), want=w, want_f32=w)]
    return out


def splitk_cases():
    """TN split-K: 2 and 3 splits whose last chunk is shorter than the others (5 stages: 3 + 2, 2 + 2 + 1), more splits than stages.  The
    operands carry a whole stage of NaN guard rows behind their last k row: a loop that runs a stage too far reads them."""
    out = []
    for tile, ring in ((64, 2), (128, 2)):
        for splits in (2, 3, 8):
            # (the last chunk of 2 + 2 + 1 and of 1 + 1 + ... is a single stage: three slots, plain loop)
            w = "g2:%dx%d:%d:128" % (tile, tile, 3 if splits != 2 else ring)
            out.append(case("splitk", TN, ACCUM_F32, 2 * tile, tile, nt=5, tile=tile, splits=splits, kguard=72, want=w))
    return out


def seg_cases():
    """both uses of a segmented B in xlnet_engine.hip, on the 64 x 64 and the 128 x 128 kernels; seg = 128 | 256 elements; the segments
    lie bseg_stride apart with NaN in the gap"""
    out = []
    for tile, want in ((64, "g2:64x64:3:128"), (128, "g2:128x128:2:128")):
        for seg in (128, 256):
            for R in (True, False):
                # NN: N = 3 * seg, k-major B cut along its columns (the fused q | k | v projection)
                out.append(case("seg", NN, ADD_RES, tile + 1, 3 * seg, nt=2, tile=tile, bseg=seg, seg_gap=40, R=R, want=want))
                # NT: K = 3 * seg, row-major B cut along k (the dgrad of the same)
                out.append(case("seg", NT, ADD_RES, tile + 1, 200, K=3 * seg, tile=tile, bseg=seg, seg_gap=40, R=R, want=want))
    return out


REFUSAL_CASES = [
    case("refuse-bseg192", NT, ADD_RES, 65, 200, K=576, tile=64, bseg=192, seg_gap=40, rc=MB_ERR_SHAPE),       # bseg % 128 != 0
    case("refuse-bseg96", NN, ADD_RES, 65, 288, nt=2, tile=64, bseg=96, seg_gap=40, rc=MB_ERR_SHAPE),          # k-major: no whole tiles per segment
    case("refuse-pn", NT, ADD_RES, 129, 200, K=384, tile=12872, bseg=128, seg_gap=40, rc=MB_ERR_SHAPE),   # a ping-pong tile by name
    case("refuse-pt", NN, ADD_RES, 257, 384, K=384, tile=25672, bseg=128, seg_gap=40, rc=MB_ERR_SHAPE),
    case("refuse-splits", NT, ADD_RES, 65, 200, K=384, tile=64, bseg=128, seg_gap=40, splits=2, rc=MB_ERR_SHAPE),
]

# The documented fallbacks ("a tile that cannot take the problem falls back to the next smaller one"): the kernel each SHOULD be.
FALLBACK_CASES = [
    # 256 x 128 ping-pong needs three stages: two run the 128 x 128 four-wave kernel (test_ops_gpu's former "shortest k range")
    case("fb-pp-2stages", TN, ACCUM_F32, 256, 128, nt=2, tile=256, want="g2:128x128:2:128", want_f32="g2:128x128:2:128"),
    case("fb-pp-2stages", NT, BIAS, 257, 200, nt=2, tile=256, want="g2:128x128:2:128", want_f32="g2:128x128:2:128"),
    # ... and has no EPI_BIAS_DROP_RES / EPI_ADD_RES / EPI_BIAS_F32 form
    case("fb-pp-epi", NT, BIAS_DROP_RES, 257, 200, nt=3, tile=256, drop=0.1, want="g2:128x128:2:128", want_f32="g2:128x128:2:128"),
    case("fb-pp-epi", NN, ADD_RES, 257, 256, nt=3, tile=256, want="g2:128x128:2:128", want_f32="g2:128x128:2:128"),
    case("fb-pp-epi", NT, BIAS_F32, 257, 200, nt=3, tile=256, want="g2:128x128:2:128", want_f32="g2:128x128:2:128"),
    # the narrow ping-pong tiles have no EPI_BIAS_GELU / EPI_BIAS_F32 / EPI_DGELU form: 64 x 64
    case("fb-pn-epi", NT, BIAS_GELU, 129, 200, nt=3, kb=256, tile=12872, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-pn-epi", NT, BIAS_F32, 129, 200, nt=3, kb=256, tile=12872, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-pn-epi", NN, DGELU, 129, 192, nt=3, kb=256, tile=12872, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-pt-epi", NT, BIAS_GELU, 257, 200, nt=3, tile=25672, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-pt-epi", NN, DGELU, 257, 192, nt=3, tile=25672, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    # ... need three stages, whole stages, and whole tiles of a k-major B
    case("fb-pn-k", NT, BIAS, 129, 200, nt=2, kb=256, tile=12872, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-pn-k", NT, BIAS, 129, 200, K=320, tile=12872, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-pt-k", NT, BIAS, 257, 200, nt=2, tile=25672, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-pn-n", NN, ADD_RES, 129, 200, nt=3, kb=256, tile=12872, want="v1:64x64:2:128", want_f32="v1:64x64:2:128"),
    # tile 0 (what the engines pass): a small problem is 12872 by the table, below its 168 tiles 64 x 64
    case("fb-auto", NT, BIAS, 300, 200, K=384, tile=0, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    case("fb-auto", NN, ADD_RES, 300, 192, K=384, tile=0, want="g2:64x64:3:128", want_f32="g2:64x64:2:128"),
    # a single stage on the two-slot 128-row kernels: three slots (bf16)
    case("fb-1stage", NT, BIAS, 129, 200, nt=1, tile=12864, want="g2:128x64:3:128", want_f32="g2:128x64:2:128"),
]


def single_cases():
    out = []
    for fam in FAMILIES:
        out += family_cases(fam)
    out += p64_cases() + epilogue_cases() + v1_cases() + splitk_cases() + seg_cases() + FALLBACK_CASES
    seen, uniq = set(), []
    for c in out:                                         # (the sweeps meet at some shapes: one case each)
        if case_id(c) not in seen:
            seen.add(case_id(c))
            uniq.append(c)
    return uniq


# grouped launch with cvalid: (tile, stages, Vp)
GROUPED = [(64, 0, 64), (64, 4, 64), (64, 5, 64), (128, 0, 128)]
GROUPED_K = [64, 128, 192]

# one rider per host: name -> (kind, launch shape, the kernel, threads and quads per thread of its adam_ride_block<NTHREADS, UNR>)
RIDE_HOSTS = {
    "g2-64": dict(kind="nn", epi=ADD_RES, M=300, N=192, K=128, want="g2ride:64x64:3:128", nthreads=256, unr=2),
    "g2-128-dgelu": dict(kind="nn", epi=DGELU, M=14 * 128 - 5, N=16 * 128, K=128, want="g2ride:128x128:2:128", nthreads=256, unr=2),
    "pn": dict(kind="nn", epi=ADD_RES, M=21 * 128 - 3, N=512, K=384, want="pnride:128x64:3:256", nthreads=512, unr=3),
    "pt": dict(kind="nn", epi=ADD_RES, M=21 * 256 - 3, N=512, K=192, want="ptride:256x64:3:128", nthreads=512, unr=3),
    "grp-128": dict(kind="grouped", tile=128, K=128, want="g2grp:128x128:2:128", nthreads=256, unr=3),
    "grp-pp": dict(kind="grouped", tile=256, K=192, want="ppgrp:256x128:3:128", nthreads=512, unr=3),
}
RIDE_BLOCKS = 8


def ride_n4s(host):
    h = RIDE_HOSTS[host]
    return [1, RIDE_BLOCKS - 1, 2 * h["nthreads"] * h["unr"] * RIDE_BLOCKS + 1]
