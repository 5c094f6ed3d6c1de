"""Operator-level machinery for the Multimodal Adaptation Gate (csrc/mag.hip, mag_fwd_impl / mag_bwd_impl in csrc/engine_common.h), shared by
tests/test_mag_op_gpu.py (the kernels, through mb_mag_forward / mb_mag_backward and the test hooks mb_debug_mag_forward_ex /
mb_debug_mag_backward_ex) and tests/test_mag_op_cpu.py (the same checker against a float32 CPU stand-in, with planted errors).  Nothing here
needs a GPU until run_gpu() is called.

Every case is a dict of plain data (case() fills the defaults): one forward and one backward.  For a case and a dtype:
  make_inputs()  text / d_out exact in the compute dtype, fp32 modalities and parameters (seeded by the case's shape, the same in both dtypes)
  reference()    float64 reference + element-wise scales (cached: cases that differ only in how they are launched share it)
  run_gpu()      the launches -> raw output buffers on the CPU (guard rows included) and the path mag_bwd_impl reported
  run_model()    the CPU stand-in: float32, hand-written backward in the kernels' form; `plant` breaks it on purpose
  check()        canaries, guard bands, finiteness, bounds -> {output: worst |err| / scale}

Reference.  oracle.mag_bert_ref.MAG in float64 on the same inputs, dropout as a multiplication with rng.keep_mult at site 1, autograd for
every gradient.  graph() below restates it so that the intermediate panels can be read (test_mag_op_cpu checks the two against each other);
for bf16 it is the same restatement with the documented storage format made explicit: text, the packed weights and the packed modalities
are bf16; the panels Ze, Zv, Za are each rounded to bf16 after an exact product and the biases are added afterwards in high precision (as
GateRow::compute does); out, the d_text-side `dep` and the three dZ panels are rounded to bf16 before the products that read them (a
straight-through rounding in the forward, a rounded gradient in the backward).  That keeps the relu decisions of the reference equal to the
kernel's except where a panel element sits on a rounding boundary: a row in which some reference |z_gate| is smaller than one ulp (of the
compute dtype) of the largest of its three summands, or whose threshold lies within two ulps of the clamp, is FRAGILE: its d_out row is
zero in the reference and in the launch, so it adds nothing to any gradient (its `out` row is still compared).  At most 1 % of a case's
rows may be fragile (test_mag_op_cpu asserts it for every case): the inputs keep |z_gate| away from zero by construction -- gate weights
scaled so that the data part of z has a standard deviation of ~0.06 under biases of 0.25 .. 1 in magnitude, text rows scaled by
1, 0.3, 0.1, 0.02 in turn so that thr (~1.7 at scale 1) lies well on either side of the clamp.

Bounds (element-wise).  An output that is a sum is judged against the magnitude summed into it, all from the reference in float64:
  dW_*            |dZ|^T |X| of its one or two problems         db_*   sum_t |dz_t|       dln_w  sum_t |dy xhat|      dln_b  sum_t |dy|
  d_text          |dZe| |We| + |dep|                            d_visual / d_acoustic     |dZ| |W| of the two halves
  out             |ref| + the row's largest |s - mu| rstd |gamma| (times the dropout multiplier: a dropped element is exactly zero)
where |dZ| and |dep| are not the absolute values of the results but the magnitude of THEIR terms (scales(): the LayerNorm adjoint's three
terms, dalpha = sum_j ds_j h_j and the two norm gradients, every difference taken as a sum).  With |result| alone a sum of one term (T = 1)
would be judged against itself, and an element whose terms cancel would set the unit for everyone.
  + |g0| where the launch accumulates into a buffer that held g0 (the add rounds to the size of the sum)
The allowed error is 4 * UNIT[dtype, output] * scale.  UNIT is not a guess: fp32 -- the largest error, in these units and over all cases,
of the same reference evaluated in float32 on the CPU; bf16 -- the storage model's own distance from the pure float64 oracle.  The kernel
sums in another order and its fp32 atomics add in no fixed order: 4 times.  UNIT is committed below (measure_units() printed it,
test_mag_op_cpu asserts that it still is the maximum); profiles/mag_op_errors.txt holds it next to the kernel's measured values."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from bert_multimodal_transformer_amd import _lib, rng

F32, BF16 = _lib.DT_F32, _lib.DT_BF16
DTS = [(F32, torch.float32), (BF16, torch.bfloat16)]
DT_NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}
MB_ERR_SHAPE, MB_ERR_ARG = 1001, 1004
PARAMS = ["W_hv", "b_hv", "W_ha", "b_ha", "W_v", "b_v", "W_a", "b_a", "ln_w", "ln_b"]
GRADS = ["dW_hv", "db_hv", "dW_ha", "db_ha", "dW_v", "db_v", "dW_a", "db_a", "dln_w", "dln_b"]       # the order of the C ABI
OUTPUTS = ["out", "d_text", "d_visual", "d_acoustic"] + GRADS
CANARY = {torch.float32: (torch.int32, 0x7FA5C3E1), torch.bfloat16: (torch.int16, 0x7FA5)}       # signalling NaNs: even `+= 0` changes them
GUARD = 3                       # guard rows behind out, d_text, d_visual, d_acoustic
SEED, STEP, SITE = 4242, 7, 1   # dropout key of every case (site 1 = MAG)
ROW_SCALES = (1.0, 0.3, 0.1, 0.02)
ALLOW = 4.0
# shapes whose first draw put more than 1 % of the rows within two bf16 ulps of the clamp (one modality column: hm_norm follows |v|)
RESEED = {(129, 768, 1, 1, "plain"): 1}
CAP = 0.01

# the largest error of the float32 CPU evaluation (f32) / of the storage model against the float64 oracle (bf16), in units of the scales
# above, over ALL_CASES -- printed by `python tests/mag_op_helpers.py`, rounded up to two digits
UNIT = {
    ("f32", "out"): 3.5e-07,    # 3.432e-07 at T193_H1024_V65_A129
    ("f32", "d_text"): 2.1e-07, # 2.044e-07 at null_beta0.001_p0.5
    ("f32", "d_visual"): 4.5e-08, # 4.472e-08 at null_beta1_p0.5
    ("f32", "d_acoustic"): 5.4e-08, # 5.313e-08 at null_beta0.001_p0.5
    ("f32", "dW_hv"): 1.1e-07,  # 1.015e-07 at null_H256_V1_A1
    ("f32", "db_hv"): 5.8e-08,  # 5.733e-08 at T1_V1_A1
    ("f32", "dW_ha"): 1.6e-07,  # 1.573e-07 at eng_T9_V1_A1_dz0
    ("f32", "db_ha"): 9.7e-08,  # 9.7e-08 at T1_V1_A1
    ("f32", "dW_v"): 3e-08,     # 2.991e-08 at T1_V1_A1
    ("f32", "db_v"): 8.3e-08,   # 8.211e-08 at null_H256_V1_A1
    ("f32", "dW_a"): 4.1e-08,   # 4.002e-08 at T1_V1_A1
    ("f32", "db_a"): 1.6e-07,   # 1.585e-07 at null_H256_V1_A1
    ("f32", "dln_w"): 2.1e-07,  # 2.049e-07 at T3
    ("f32", "dln_b"): 1.3e-07,  # 1.277e-07 at eng_T9_V35_A74_dz0
    ("bf16", "out"): 0.0047,     # 0.004698 at eng_T193_V35_A74_dz0
    ("bf16", "d_text"): 0.0048,  # 0.004741 at null_H256_V1_A1
    ("bf16", "d_visual"): 0.00023, # 0.0002241 at null_beta1_p0
    ("bf16", "d_acoustic"): 0.00025, # 0.0002433 at null_beta0.001_p0.5
    ("bf16", "dW_hv"): 0.003,    # 0.002944 at null_H256_V1_A1
    ("bf16", "db_hv"): 0.002,    # 0.001991 at T1_V1_A1
    ("bf16", "dW_ha"): 0.0037,   # 0.00368 at T1_V1_A1
    ("bf16", "db_ha"): 0.0026,   # 0.002538 at T1_V1_A1
    ("bf16", "dW_v"): 0.00074,   # 0.0007308 at T1_V1_A1
    ("bf16", "db_v"): 0.00037,   # 0.0003609 at eng_T9_V1_A1_dz0
    ("bf16", "dW_a"): 0.00093,   # 0.0009274 at T1_V1_A1
    ("bf16", "db_a"): 0.00027,   # 0.0002679 at eng_T9_V1_A1_dz0
    ("bf16", "dln_w"): 0.0024,   # 0.002314 at eng_T9_V1_A1_dz0
    ("bf16", "dln_b"): 0,        # 0 at T1
}


def unit(dtype_name, output):
    """a bf16 launch accumulates in fp32 like an fp32 one: where the storage model is exact (dln_b: a plain sum of bf16 values) or nearly
    so, the fp32 unit holds"""
    return max(UNIT[dtype_name, output], UNIT["f32", output])


# ------------------------------------------------------------------------------------------------------------------------------ cases
def case(name, T=65, H=768, V=47, A=74, beta=1.0, p=0.5, kind="plain", g0=False, no_dv=False, no_da=False, hook=False, text_padded=0,
         pads_clean=0, slabs=0, dw_zero=0, path=None):
    """kind: "plain" | "null" (null rows, dead gate columns, faint modality rows).  g0: the ten gradient buffers start from a non-zero
    pattern.  hook: through mb_debug_mag_*_ex with text_padded .. dw_zero; path = what mag_bwd_impl must report (path_table())."""
    return dict(name=name, T=T, H=H, V=V, A=A, beta=beta, p=p, kind=kind, g0=g0, no_dv=no_dv, no_da=no_da, hook=hook,
                text_padded=text_padded, pads_clean=pads_clean, slabs=slabs, dw_zero=dw_zero, path=path)


def path_table(tdt, T, text_padded):
    """(grouped, direct, tile) of mag_bwd_impl, from reading it with gemm_grouped_tn_ok (csrc/gemm.hip) and mag_wgrad_tile:
    the tile is 64 unless MB_MAG_WGRAD_TILE=128 (out of scope).  Every M (2H, H), N (H, Vp, Ap), leading dimension and pointer of the
    three / six problems is a multiple of 64 elements for any H in {256 .. 1024}, V, A (the widths are padded to the tile and every direct
    problem carries cvalid = V | A | H > 0, <= N), so the only condition that can fail is K % BKE (BKE = 64 elements in bf16, 32 in fp32):
    K = Tp = align_up(T, 64) with text_padded -- always whole stages -- and K = T without.  Without text_padded the launch is never grouped
    (`grouped = text_padded && ...`).  direct = grouped (MB_MAG_WGRAD_DIRECT=0 is out of scope)."""
    grouped = 1 if text_padded else 0
    return (grouped, grouped, 64)


def _id(c):
    return c["name"]


VA_LIST = [(47, 74), (35, 74), (1, 1), (64, 128), (65, 129)]


def _standalone_cases():
    cs = [case("T%d" % T, T=T) for T in (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129, 193)]
    cs += [case("H%d_T%d" % (H, T), T=T, H=H) for H in (256, 512, 768, 1024) for T in (9, 65) if (H, T) != (768, 65)]
    cs += [case("V%d_A%d" % va, V=va[0], A=va[1]) for va in VA_LIST[1:]]
    cs += [case("beta1e-3", beta=1e-3), case("beta64", beta=64.0), case("p0", p=0.0), case("p0.1", p=0.1)]
    cs += [case("null_beta%g_p%g" % (b, p), T=21, beta=b, p=p, kind="null") for b in (1.0, 1e-3) for p in (0.0, 0.5)]
    # combinations: the smallest of everything; the widest rows with no pad column to spare at four k stages; an odd T with full widths
    cs += [case("T1_V1_A1", T=1, V=1, A=1), case("T193_H1024_V65_A129", T=193, H=1024, V=65, A=129),
           case("T63_H256_V64_A128_p0.1", T=63, H=256, V=64, A=128, p=0.1), case("null_H1024", T=21, H=1024, kind="null"),
           case("null_H256_V1_A1", T=21, H=256, V=1, A=1, kind="null")]
    # contract of the C ABI
    cs += [case("g0", g0=True), case("g0_T9_H1024", T=9, H=1024, g0=True), case("no_dv", no_dv=True), case("no_da", no_da=True),
           case("no_dv_no_da", no_dv=True, no_da=True)]
    return cs


def _engine_cases():
    cs = []
    eng = dict(no_dv=True, no_da=True, hook=True, text_padded=1, pads_clean=1, slabs=1, path=(1, 1, 64))
    for T in (1, 9, 64, 65, 129, 193):
        for V, A in VA_LIST:
            cs += [case("eng_T%d_V%d_A%d_dz%d" % (T, V, A, dz), T=T, V=V, A=A, g0=not dz, dw_zero=dz, **eng) for dz in (0, 1)]
    for H in (256, 1024):
        cs += [case("eng_H%d_dz%d" % (H, dz), H=H, g0=not dz, dw_zero=dz, **eng) for dz in (0, 1)]
    # the hook on the stand-alone operator's path (three launches into packed scratch + unpack), slabs on and off, with the modality gradients
    cs += [case("hook_unpadded_T%d_s%d" % (T, s), T=T, hook=True, slabs=s, g0=True, path=(0, 0, 64)) for T in (64, 65) for s in (0, 1)]
    return cs


STANDALONE_CASES = _standalone_cases()
ENGINE_CASES = _engine_cases()
ALL_CASES = STANDALONE_CASES + ENGINE_CASES
PLANTS = ["thr_eps_1e-5", "no_hm_replacement", "no_clamp", "no_dnorm_e", "gate_ge", "ln_eps_1e-12", "no_dropout_bwd", "last_row_dropped",
          "dW_hv_shifted", "bias_grad_stored"]


# ----------------------------------------------------------------------------------------------------------------------------- inputs
def _key(c):
    return (c["T"], c["H"], c["V"], c["A"], c["beta"], c["p"], c["kind"])


def null_rows(T):
    """(hm-null rows, text-null rows, faint rows) of the null case: a wave of the backward takes rows (2k, 2k + 1).  Pairs: (0, 1) null /
    ordinary, (2, 3) ordinary / null, (4, 5) null / null with one of each kind, (6, 7) null / null with row 6 in both sets; the last row of
    the odd T is hm-null; row 9 has a modality row of ~1e-4 (hm_norm tiny but not zero)."""
    assert T % 2 == 1 and T >= 13
    return [0, 4, 6, 7, T - 1], [3, 5, 6], [9]


def make_inputs(c, tdt):
    T, H, V, A = c["T"], c["H"], c["V"], c["A"]
    g = torch.Generator().manual_seed(zlib.crc32(repr((T, H, V, A, c["kind"])).encode()) + RESEED.get((T, H, V, A, c["kind"]), 0))

    def u(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1

    def away(n):          # magnitudes 0.25 .. 1, random sign
        x = u(n)
        return torch.sign(x) * (0.25 + 0.75 * u(n).abs())

    I = {}
    I["W_hv"] = torch.cat([u(H, V) * 0.06 / math.sqrt(V), u(H, H) * 0.08 / math.sqrt(H)], 1)
    I["b_hv"] = away(H)
    I["W_ha"] = torch.cat([u(H, A) * 0.06 / math.sqrt(A), u(H, H) * 0.08 / math.sqrt(H)], 1)
    I["b_ha"] = away(H)
    I["W_v"] = u(H, V) / math.sqrt(V)
    I["b_v"] = u(H) * 0.1
    I["W_a"] = u(H, A) / math.sqrt(A)
    I["b_a"] = u(H) * 0.1
    I["ln_w"] = 1 + 0.2 * u(H)
    I["ln_b"] = 0.2 * u(H)
    scale = torch.tensor([ROW_SCALES[t % len(ROW_SCALES)] for t in range(T)], dtype=torch.float64)
    text = u(T, H) * 1.5
    vis, aco = u(T, V) * 2, u(T, A) * 2
    if c["kind"] == "null":
        hm0, e0, faint = null_rows(T)
        I["b_v"].zero_(); I["b_a"].zero_()
        scale[0] = 0.02; scale[4] = 1.0; scale[9] = 0.02
        vis[hm0] = 0; aco[hm0] = 0
        vis[faint] *= 1e-4; aco[faint] *= 1e-4
        scale[e0] = 0.0
        for j in (0, 5, H - 1):           # gate columns whose pre-activation is exactly zero in every row: relu'(0) = 0
            I["W_hv"][j] = 0; I["b_hv"][j] = 0
        I["W_ha"][1] = 0; I["b_ha"][1] = 0
    text = text * scale[:, None]
    I = {k: v.float() for k, v in I.items()}
    I["text"] = text.float().to(tdt)
    I["visual"], I["acoustic"] = vis.float(), aco.float()
    I["d_out"] = u(T, H).float().to(tdt)
    key = rng.make_key(SEED, STEP, SITE, c["p"])
    I["mask"] = torch.from_numpy(rng.keep_mult(T * H, key)).view(T, H)
    return I


def g0_pattern(name, shape):
    n = int(np.prod(shape))
    i = torch.arange(n, dtype=torch.float32) + len(name)
    return (((i % 7) + 1) / 64 * (1 - 2 * (i % 2))).view(shape)


# -------------------------------------------------------------------------------------------------------------------------- reference
def rb(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _Store(torch.autograd.Function):
    """a tensor held in bf16: the value rounded on the way forward (fwd), the gradient rounded on the way back (bwd)"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return rb(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (rb(g) if ctx.bwd else g), None, None


def graph(L, mask, beta, store):
    """modeling.py:25-49 regrouped by input as the kernels do it (no concatenation); L: leaves in the working dtype.  store: bf16 storage
    made explicit.  -> out and the intermediates the scales and the fragile-row rule read."""
    r = _Store.apply if store else (lambda x, fwd, bwd: x)
    V, A = L["visual"].shape[1], L["acoustic"].shape[1]
    H = L["text"].shape[1]
    e = L["text"]
    W_hv, W_ha, W_v, W_a = (r(L[n], True, False) for n in ("W_hv", "W_ha", "W_v", "W_a"))
    v, a = r(L["visual"], True, False), r(L["acoustic"], True, False)
    m = {}
    m["Ze_gv"], m["Ze_ga"] = r(e @ W_hv[:, V:].T, True, True), r(e @ W_ha[:, A:].T, True, True)
    m["Zv_g"], m["Zv_p"] = r(v @ W_hv[:, :V].T, True, True), r(v @ W_v.T, True, True)
    m["Za_g"], m["Za_p"] = r(a @ W_ha[:, :A].T, True, True), r(a @ W_a.T, True, True)
    m["e_d"] = e_d = r(e, False, True) if store else e.clone()                               # the text row as the gate kernel reads it: its gradient is `dep`
    m["z_gv"] = m["Ze_gv"] + m["Zv_g"] + L["b_hv"]
    m["z_ga"] = m["Ze_ga"] + m["Za_g"] + L["b_ha"]
    m["pv"], m["pa"] = m["Zv_p"] + L["b_v"], m["Za_p"] + L["b_a"]
    h = F.relu(m["z_gv"]) * m["pv"] + F.relu(m["z_ga"]) * m["pa"]           # modeling.py:27-30
    en, hn = e_d.norm(2, dim=-1), h.norm(2, dim=-1)                        # :32-33
    m["h"], m["en"], m["hn"] = h, en, hn
    hn = torch.where(hn == 0, torch.ones_like(hn), hn)                    # :35-36
    m["thr"] = en / (hn + 1e-6) * beta                                    # :38
    alpha = torch.min(m["thr"], torch.ones_like(m["thr"])).unsqueeze(-1)  # :40-43
    s = alpha * h + e_d                                                   # :45,48
    mu = s.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((s - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    m["xhat"], m["rstd"], m["alpha"], m["mu"] = (s - mu) * rstd, rstd, alpha, mu
    y = (m["xhat"] * L["ln_w"] + L["ln_b"]) * mask                        # :47-49 (LayerNorm eps 1e-5, dropout as a multiplier)
    m["v"], m["a"], m["Ws"] = v, a, (W_hv, W_ha, W_v, W_a)
    for k in ("z_gv", "z_ga", "pv", "pa", "e_d"):
        m[k].retain_grad()
    return r(y, True, False), m


def _leaves(I, wdt):
    L = {k: I[k].to(wdt).clone().requires_grad_(True) for k in PARAMS + ["text", "visual", "acoustic"]}
    return L


def evaluate(I, beta, store, wdt, keep=None):
    """forward + autograd backward of graph() -> ({output: tensor in wdt}, intermediates)"""
    L = _leaves(I, wdt)
    out, m = graph(L, I["mask"].to(wdt), beta, store)
    dout = I["d_out"].to(wdt)
    if keep is not None:
        dout = dout * keep[:, None].to(wdt)
    (out * dout).sum().backward()
    res = {"out": out.detach(), "d_text": rb(L["text"].grad) if store else L["text"].grad, "d_visual": L["visual"].grad,
           "d_acoustic": L["acoustic"].grad}
    for n, p in zip(GRADS, PARAMS):
        res[n] = L[p].grad
    m["dout"] = dout
    return res, m


def oracle(I, beta, keep=None):
    """oracle.mag_bert_ref.MAG itself, float64: the reference of the fp32 launches"""
    from oracle import mag_bert_ref as R
    H, V, A = I["text"].shape[1], I["visual"].shape[1], I["acoustic"].shape[1]
    o = R.MAG(H, beta, 0.0, V, A).double()
    o.load_state_dict({"W_hv.weight": I["W_hv"].double(), "W_hv.bias": I["b_hv"].double(), "W_ha.weight": I["W_ha"].double(),
                       "W_ha.bias": I["b_ha"].double(), "W_v.weight": I["W_v"].double(), "W_v.bias": I["b_v"].double(),
                       "W_a.weight": I["W_a"].double(), "W_a.bias": I["b_a"].double(), "LayerNorm.weight": I["ln_w"].double(),
                       "LayerNorm.bias": I["ln_b"].double()})
    x = [I[k].double().clone().requires_grad_(True) for k in ("text", "visual", "acoustic")]
    out = o(*x) * I["mask"].double()
    dout = I["d_out"].double()
    if keep is not None:
        dout = dout * keep[:, None].double()
    (out * dout).sum().backward()
    res = {"out": out.detach(), "d_text": x[0].grad, "d_visual": x[1].grad, "d_acoustic": x[2].grad}
    P = dict(o.named_parameters())
    for n, k in zip(GRADS, ("W_hv.weight", "W_hv.bias", "W_ha.weight", "W_ha.bias", "W_v.weight", "W_v.bias", "W_a.weight", "W_a.bias",
                            "LayerNorm.weight", "LayerNorm.bias")):
        res[n] = P[k].grad
    return res


def _ulp(x, tdt):
    """one unit in the last place of |x| in tdt (0 at 0)"""
    bits = 7 if tdt == torch.bfloat16 else 23
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp_min(1e-300))) - bits), torch.zeros_like(x))


def fragile_rows(m, I, tdt):
    """bool [T]: rows whose gate decisions or clamp decision a last-place difference could turn (module docstring)"""
    bad = torch.zeros(m["thr"].shape[0], dtype=torch.bool)
    for z, parts in ((m["z_gv"], (m["Ze_gv"], m["Zv_g"], I["b_hv"])), (m["z_ga"], (m["Ze_ga"], m["Za_g"], I["b_ha"]))):
        big = torch.stack([p.detach().double().abs().expand_as(z) for p in parts]).amax(0)
        bad |= (z.detach().abs() < _ulp(big, tdt)).any(-1)
    bad |= (m["thr"].detach() - 1).abs() < 2 * _ulp(torch.ones(1, dtype=torch.float64), tdt)
    return bad


def scales(res, m, I, beta):
    """element-wise magnitude summed into every output (module docstring), float64, from one evaluation"""
    W_hv, W_ha, W_v, W_a = (w.detach().abs() for w in m["Ws"])
    V, A = I["visual"].shape[1], I["acoustic"].shape[1]
    ae, av, aa = I["text"].double().abs(), m["v"].detach().abs(), m["a"].detach().abs()
    mask = I["mask"].double()
    dy = (m["dout"] * mask).abs()
    # the magnitude of the terms of one dZ element, carried through the row's adjoint: ds = (dxh - mean(dxh) - xhat mean(dxh xhat)) rstd,
    # dalpha = sum ds h, dh = alpha ds + (d hm_norm / hm_norm) h, dep = ds + (d em_norm / em_norm) e -- every difference as a sum
    en, hn, thr = (m[k].detach() for k in ("en", "hn", "thr"))
    alpha, rstd = m["alpha"].detach(), m["rstd"].detach()
    Pv, Pa = av @ W_v.T + I["b_v"].double().abs(), aa @ W_a.T + I["b_a"].double().abs()         # (a panel element: |X| |W|^T, not |X W^T|)
    Gv = (m["z_gv"].detach() > 0) * (ae @ W_hv[:, V:].T + av @ W_hv[:, :V].T + I["b_hv"].double().abs())
    Ga = (m["z_ga"].detach() > 0) * (ae @ W_ha[:, A:].T + aa @ W_ha[:, :A].T + I["b_ha"].double().abs())
    h = Gv * Pv + Ga * Pa
    xh = (alpha * h + ae + m["mu"].detach().abs()) * rstd                   # the terms of xhat = (alpha h + e - mu) rstd
    dxh = dy * I["ln_w"].double().abs()
    Ds = (dxh + dxh.mean(-1, keepdim=True) + xh * (dxh * xh).mean(-1, keepdim=True)) * rstd
    Dthr = torch.where(thr < 1, (Ds * h).sum(-1), torch.zeros_like(thr))
    inv = 1.0 / (torch.where(hn == 0, torch.ones_like(hn), hn) + 1e-6)
    Dhn = torch.where(hn > 0, Dthr * en * beta * inv * inv / hn.clamp_min(1e-300), torch.zeros_like(hn))
    Den = torch.where(en > 0, Dthr * beta * inv / en.clamp_min(1e-300), torch.zeros_like(en))
    Dh = alpha * Ds + Dhn[:, None] * h
    dzgv, dzga = (Gv > 0) * Dh * Pv, (Ga > 0) * Dh * Pa
    dpv, dpa = Dh * Gv, Dh * Ga
    S = {}
    S["out"] = res["out"].abs() + (m["xhat"].detach() * I["ln_w"].double()).abs().amax(-1, keepdim=True) * mask
    S["d_text"] = dzgv @ W_hv[:, V:] + dzga @ W_ha[:, A:] + Ds + Den[:, None] * ae
    S["d_visual"] = dzgv @ W_hv[:, :V] + dpv @ W_v
    S["d_acoustic"] = dzga @ W_ha[:, :A] + dpa @ W_a
    S["dW_hv"] = torch.cat([dzgv.T @ av, dzgv.T @ ae], 1)
    S["dW_ha"] = torch.cat([dzga.T @ aa, dzga.T @ ae], 1)
    S["dW_v"], S["dW_a"] = dpv.T @ av, dpa.T @ aa
    S["db_hv"], S["db_ha"], S["db_v"], S["db_a"] = dzgv.sum(0), dzga.sum(0), dpv.sum(0), dpa.sum(0)
    S["dln_w"], S["dln_b"] = (dy * xh).sum(0), dy.sum(0)
    return S


@functools.lru_cache(maxsize=16)
def _reference(key, tdt):
    c = dict(zip(("T", "H", "V", "A", "beta", "p", "kind"), key))
    I = make_inputs(c, tdt)
    store = tdt == torch.bfloat16
    res, m = evaluate(I, c["beta"], store, torch.float64)
    keep = (~fragile_rows(m, I, tdt)).double()
    if bool((keep == 0).any()):
        res, m = evaluate(I, c["beta"], store, torch.float64, keep)
    S = scales(res, m, I, c["beta"])
    I["keep"] = keep
    if not store:
        res = oracle(I, c["beta"], keep)          # fp32 launches: the oracle itself (graph() supplies the scales only)
    return dict(I=I, ref=res, S=S, thr=m["thr"].detach(), fragile=int((keep == 0).sum()))


def reference(c, tdt):
    """-> dict(I inputs (with the row mask `keep`), ref {output: float64}, S scales, thr, fragile row count);
    shared among the cases with the same shapes and never changed"""
    return _reference(_key(c), tdt)


def units(got, ref, S):
    """{output: max over elements of |got - ref| / scale}; an error where the scale is zero counts as infinite"""
    u = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        err = (got[k].double() - ref[k].double()).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / S[k].clamp_min(1e-300))
        u[k] = float(ratio.max()) if ratio.numel() else 0.0
    return u


def cpu_unit(c, tdt):
    """what UNIT is the maximum of: fp32 -- the reference evaluated in float32; bf16 -- the storage model against the float64 oracle"""
    R = reference(c, tdt)
    if tdt == torch.float32:
        got, _ = evaluate(R["I"], c["beta"], False, torch.float32, R["I"]["keep"])
        return units(got, R["ref"], R["S"])
    return units(R["ref"], oracle(R["I"], c["beta"], R["I"]["keep"]), R["S"])


# ------------------------------------------------------------------------------------------------------------------------------ check
def _canary(shape, tdt):
    it, val = CANARY[tdt]
    return torch.full(shape, val, dtype=it).view(tdt)


def _is_canary(t):
    it, val = CANARY[t.dtype]
    return t.contiguous().view(it) == val


def alloc_outputs(c, tdt):
    """the output buffers of one case as the launch finds them: canaries (with guard rows) where the operator stores, zeros / g0 / canaries
    in the ten gradient buffers"""
    T, H, V, A = c["T"], c["H"], c["V"], c["A"]
    B = {"out": _canary((T + GUARD, H), tdt), "d_text": _canary((T + GUARD, H), tdt),
         "d_visual": None if c["no_dv"] else _canary((T + GUARD, V), torch.float32),
         "d_acoustic": None if c["no_da"] else _canary((T + GUARD, A), torch.float32)}
    shapes = {"dW_hv": (H, V + H), "dW_ha": (H, A + H), "dW_v": (H, V), "dW_a": (H, A)}
    for n in GRADS:
        shape = shapes.get(n, (H,))
        if c["dw_zero"] and n in shapes:
            B[n] = _canary(shape, torch.float32)           # stored, never read
        else:
            B[n] = g0_pattern(n, shape) if c["g0"] else torch.zeros(shape)
    return B


def check(c, tdt, got, path=None):
    """canaries, guard bands, finiteness, then the bounds; -> {output: worst |err| / scale}.  Raises AssertionError with every miss."""
    R = reference(c, tdt)
    T = c["T"]
    name = DT_NAME[tdt]
    bad = []
    if c["path"] is not None or path is not None:
        if tuple(path) != tuple(c["path"]) or tuple(path) != path_table(tdt, T, c["text_padded"]):
            bad.append("path %r, expected %r" % (path, c["path"]))
    vals = {}
    for k in ("out", "d_text", "d_visual", "d_acoustic"):
        if got.get(k) is None:
            assert (k == "d_visual" and c["no_dv"]) or (k == "d_acoustic" and c["no_da"]), k
            continue
        if not bool(_is_canary(got[k][T:]).all()):
            bad.append("%s: guard rows written" % k)
        vals[k] = got[k][:T]
    S = dict(R["S"])
    ref = dict(R["ref"])
    for n in GRADS:
        vals[n] = got[n]
        stored = c["dw_zero"] and n.startswith("dW_")
        if c["g0"] and not stored:
            g0 = g0_pattern(n, got[n].shape).double()
            ref[n] = ref[n] + g0
            S[n] = S[n] + g0.abs()
    for k, v in vals.items():
        if not bool(torch.isfinite(v.float()).all()):
            bad.append("%s: %d non-finite elements" % (k, int((~torch.isfinite(v.float())).sum())))
            vals[k] = None
        if not bool(torch.isfinite(ref[k]).all()):
            bad.append("%s: the reference is not finite" % k)
    u = units(vals, ref, S)
    for k, x in u.items():
        if not x <= ALLOW * unit(name, k):
            bad.append("%s: |err| / scale = %.3g > %g * %.3g" % (k, x, ALLOW, unit(name, k)))
    assert not bad, "%s %s: " % (c["name"], name) + "; ".join(bad)
    return u


# ---------------------------------------------------------------------------------------------------------------------------- the GPU
def align_up(x, a):
    return (x + a - 1) // a * a


def ws_layout(dt, T, H, V, A):
    """byte offsets of csrc/engine_common.h MagWs (every piece aligned to 256 bytes) -> ({name: (offset, bytes)}, total, Vp, Ap)"""
    es = 2 if dt == BF16 else 4
    Tp, Vp, Ap = align_up(T, 64), align_up(V, 64), align_up(A, 64)
    sizes = [("We", 2 * H * H * es), ("Wv", 2 * H * Vp * es), ("Wa", 2 * H * Ap * es), ("vp", Tp * Vp * es), ("ap", Tp * Ap * es),
             ("Ze", Tp * 2 * H * es), ("Zv", Tp * 2 * H * es), ("Za", Tp * 2 * H * es), ("mean", Tp * 4), ("rstd", Tp * 4),
             ("dZe", Tp * 2 * H * es), ("dZv", Tp * 2 * H * es), ("dZa", Tp * 2 * H * es), ("dep", Tp * H * es),
             ("dWe", 2 * H * H * 4), ("dWv", 2 * H * Vp * 4), ("dWa", 2 * H * Ap * 4), ("dvp", Tp * Vp * 4), ("dap", Tp * Ap * 4)]
    off, lay = 0, {}
    for n, b in sizes:
        lay[n] = (off, b)
        off = align_up(off + b, 256)
    return lay, off, Vp, Ap


def clear_pad_rows(ws, dt, T, H, V, A):
    """what the engines' mag_clear_pad_rows does: rows [T, Tp) of the packed modalities and of the three dZ panels"""
    lay, _, Vp, Ap = ws_layout(dt, T, H, V, A)
    es = 2 if dt == BF16 else 4
    Tp = align_up(T, 64)
    for n, cols in (("vp", Vp), ("ap", Ap), ("dZe", 2 * H), ("dZv", 2 * H), ("dZa", 2 * H)):
        o = lay[n][0]
        ws[o + T * cols * es: o + Tp * cols * es] = 0


def _dropkey(p):
    return _lib.make_dropkey(SEED, STEP, SITE, p) if p > 0 else _lib.no_drop()


def gpu_forward(c, dt, tdt, I, dev, ws=None, out=None):
    """mb_mag_forward (or the hook) of the case on a workspace of 0xFF bytes (NaN in either dtype) -> (device inputs, ws, out)"""
    L = _lib.lib()
    T, H, V, A = c["T"], c["H"], c["V"], c["A"]
    nbytes = L.mb_mag_workspace_bytes(dt, T, H, V, A)
    assert nbytes == ws_layout(dt, T, H, V, A)[1]
    if ws is None:
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        if c["pads_clean"]:
            clear_pad_rows(ws, dt, T, H, V, A)
    D = {k: I[k].to(dev) for k in PARAMS + ["visual", "acoustic", "d_out"]}
    text = I["text"]
    if c["text_padded"]:          # rows [T, Tp) meet zero dZ rows in the weight-gradient launch: large finite values change nothing
        text = torch.cat([text, torch.full((align_up(T, 64) - T, H), 1e4, dtype=tdt)])
    D["text"] = text.to(dev)
    if out is None:
        out = _canary((T + GUARD, H), tdt).to(dev)
    args = [dt, _lib.ptr(D["text"]), _lib.ptr(D["visual"]), _lib.ptr(D["acoustic"])] + [_lib.ptr(D[k]) for k in PARAMS] + \
           [float(c["beta"]), _dropkey(c["p"]), _lib.ptr(out), _lib.ptr(ws), T, H, V, A]
    st = torch.cuda.current_stream(dev).cuda_stream
    if c["hook"]:
        rc = L.mb_debug_mag_forward_ex(*args, c["pads_clean"], st)
    else:
        rc = L.mb_mag_forward(*args, st)
    assert rc == 0, rc
    return D, ws, out


def run_gpu(c, tdt, dev="cuda", ws=None, keep_ws=False):
    """one forward and one backward of the case -> ({output: raw buffer on the CPU}, path or None).  ws: run on this workspace as it is
    (at least as large as the case's) instead of a fresh one; keep_ws: hand the workspace back as got["ws"]"""
    L = _lib.lib()
    dt = BF16 if tdt == torch.bfloat16 else F32
    R = reference(c, tdt)
    I = dict(R["I"])
    I["d_out"] = (I["d_out"].float() * I["keep"][:, None].float()).to(tdt)       # fragile rows (none in most cases): no gradient
    T, H, V, A = c["T"], c["H"], c["V"], c["A"]
    D, ws, out = gpu_forward(c, dt, tdt, I, dev, ws=ws)
    B = {k: (None if v is None else v.to(dev)) for k, v in alloc_outputs(c, tdt).items()}
    B["out"] = out
    st = torch.cuda.current_stream(dev).cuda_stream
    key = _dropkey(c["p"])
    tail = [_lib.ptr(ws), _lib.ptr(B["d_text"]), _lib.ptr(B["d_visual"]), _lib.ptr(B["d_acoustic"])] + [_lib.ptr(B[n]) for n in GRADS] + \
           [T, H, V, A]
    path = None
    if c["hook"]:
        slab = torch.full((max(1, L.mb_debug_mag_slab_bytes(T, H) // 4),), float("nan"), device=dev) if c["slabs"] else None
        pout = (C.c_int * 3)(-1, -1, -1)
        rc = L.mb_debug_mag_backward_ex(dt, _lib.ptr(D["d_out"]), _lib.ptr(D["text"]), _lib.ptr(D["b_hv"]), _lib.ptr(D["b_ha"]),
                                        _lib.ptr(D["b_v"]), _lib.ptr(D["b_a"]), _lib.ptr(D["ln_w"]), float(c["beta"]), key, *tail,
                                        c["text_padded"], c["pads_clean"], c["slabs"], _lib.ptr(slab),
                                        0 if slab is None else slab.numel() * 4, c["dw_zero"], pout, st)
        path = tuple(pout)
    else:
        rc = L.mb_mag_backward(dt, _lib.ptr(D["d_out"]), _lib.ptr(D["text"]), _lib.ptr(D["W_hv"]), _lib.ptr(D["b_hv"]),
                               _lib.ptr(D["W_ha"]), _lib.ptr(D["b_ha"]), _lib.ptr(D["W_v"]), _lib.ptr(D["b_v"]), _lib.ptr(D["W_a"]),
                               _lib.ptr(D["b_a"]), _lib.ptr(D["ln_w"]), float(c["beta"]), key, *tail, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = {k: (None if v is None else v.cpu()) for k, v in B.items()}
    if keep_ws:
        got["ws"] = ws
    return got, path


def run_reused_workspace(tdt, dev="cuda"):
    """forward + backward at T = 65, then forward + backward at T = 9 on the SAME workspace -> (the second pair's outputs, the outputs of
    the same case on a fresh workspace); the reused run is checked against the bounds on the way"""
    big, small = case("T65", T=65), case("T9", T=9)
    first, _ = run_gpu(big, tdt, dev, keep_ws=True)
    reused, _ = run_gpu(small, tdt, dev, ws=first["ws"])
    check(small, tdt, reused)
    fresh, _ = run_gpu(small, tdt, dev)
    return reused, fresh


def arg_refusals(dt):
    """[(what, return code)]: slabs asked for without scratch, or with too little -- MB_ERR_ARG before anything is launched"""
    L = _lib.lib()
    head = [dt] + [None] * 7 + [1.0, _lib.no_drop()] + [None] * 14 + [65, 768, 47, 74, 1, 1, 1]
    need = L.mb_debug_mag_slab_bytes(65, 768)
    return [("no scratch", L.mb_debug_mag_backward_ex(*(head + [None, need, 0, None, None]))),
            ("short scratch", L.mb_debug_mag_backward_ex(*(head + [C.c_void_p(256), need - 4, 0, None, None])))]


def refusals(dt):
    """[(what, return code)] of shapes the operator does not take: every call must return MB_ERR_SHAPE before it reads a pointer"""
    L = _lib.lib()
    res = []
    for T, H, V, A in ((8, 768, 0, 74), (8, 768, 47, 0), (8, 128, 47, 74), (8, 1280, 47, 74), (8, 800, 47, 74)):
        tag = "H%d_V%d_A%d" % (H, V, A)
        fwd = [dt] + [None] * 13 + [1.0, _lib.no_drop(), None, None, T, H, V, A]
        res.append(("forward " + tag, L.mb_mag_forward(*fwd, None)))
        res.append(("forward hook " + tag, L.mb_debug_mag_forward_ex(*fwd, 0, None)))
        res.append(("backward " + tag, L.mb_mag_backward(*([dt] + [None] * 11 + [1.0, _lib.no_drop()] + [None] * 14 + [T, H, V, A, None]))))
        res.append(("backward hook " + tag, L.mb_debug_mag_backward_ex(*([dt] + [None] * 7 + [1.0, _lib.no_drop()] + [None] * 14 +
                                                                         [T, H, V, A, 1, 1, 0, None, 0, 0, None, None]))))
    return res


# -------------------------------------------------------------------------------------------------------------------- the CPU stand-in
def run_model(c, tdt, plant=None):
    """float32 stand-in of the operator in the kernels' form (hand-written backward), written into the buffers run_gpu() returns"""
    assert tdt == torch.float32
    R = reference(c, tdt)
    I = R["I"]
    T, H, V, A = c["T"], c["H"], c["V"], c["A"]
    beta = np.float32(c["beta"])
    e, v, a = I["text"].float(), I["visual"], I["acoustic"]
    W_hv, W_ha, W_v, W_a = I["W_hv"], I["W_ha"], I["W_v"], I["W_a"]
    mask = I["mask"]
    dout = I["d_out"].float() * I["keep"][:, None].float()
    n = T - 1 if plant == "last_row_dropped" else T
    e, v, a, mask, dout = e[:n], v[:n], a[:n], mask[:n], dout[:n]
    zgv = e @ W_hv[:, V:].T + v @ W_hv[:, :V].T + I["b_hv"]
    zga = e @ W_ha[:, A:].T + a @ W_ha[:, :A].T + I["b_ha"]
    pv, pa = v @ W_v.T + I["b_v"], a @ W_a.T + I["b_a"]
    gv, ga = zgv.clamp_min(0), zga.clamp_min(0)
    h = gv * pv + ga * pa
    en, hn = e.pow(2).sum(-1).sqrt(), h.pow(2).sum(-1).sqrt()
    hn0 = hn if plant == "no_hm_replacement" else torch.where(hn == 0, torch.ones_like(hn), hn)
    eps = 1e-5 if plant == "thr_eps_1e-5" else 1e-6
    thr = en / (hn0 + eps) * beta
    alpha = thr if plant == "no_clamp" else thr.clamp_max(1.0)
    s = alpha[:, None] * h + e
    mu = s.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((s - mu) ** 2).mean(-1, keepdim=True) + (1e-12 if plant == "ln_eps_1e-12" else 1e-5))
    xh = (s - mu) * rs
    out = (xh * I["ln_w"] + I["ln_b"]) * mask
    # backward, as mag_gate_bwd_kernel
    dy = dout if plant == "no_dropout_bwd" else dout * mask
    dxh = dy * I["ln_w"]
    m1, m2 = dxh.mean(-1, keepdim=True), (dxh * xh).mean(-1, keepdim=True)
    ds = (dxh - m1 - xh * m2) * rs
    dalpha = (ds * h).sum(-1)
    if plant == "no_clamp":
        dthr = dalpha
    else:
        dthr = torch.where(thr < 1, dalpha, torch.where(thr == 1, 0.5 * dalpha, torch.zeros_like(dalpha)))
    inv = 1.0 / (hn0 + eps)
    den = dthr * beta * inv
    dhn = torch.where(hn == 0, torch.zeros_like(hn), -dthr * en * beta * inv * inv)
    ce = torch.where(en > 0, den / en.clamp_min(1e-30), torch.zeros_like(en))
    ch = torch.where(hn > 0, dhn / hn.clamp_min(1e-30), torch.zeros_like(hn))
    if plant == "no_dnorm_e":
        ce = torch.zeros_like(ce)
    dh = alpha[:, None] * ds + ch[:, None] * h
    dE = ds + ce[:, None] * e
    on_v, on_a = (zgv >= 0, zga >= 0) if plant == "gate_ge" else (zgv > 0, zga > 0)
    dzgv, dzga = torch.where(on_v, dh * pv, torch.zeros_like(dh)), torch.where(on_a, dh * pa, torch.zeros_like(dh))
    dpv, dpa = dh * gv, dh * ga
    G = {"dW_hv": torch.cat([dzgv.T @ v, dzgv.T @ e], 1), "dW_ha": torch.cat([dzga.T @ a, dzga.T @ e], 1), "dW_v": dpv.T @ v,
         "dW_a": dpa.T @ a, "db_hv": dzgv.sum(0), "db_ha": dzga.sum(0), "db_v": dpv.sum(0), "db_a": dpa.sum(0),
         "dln_w": (dy * xh).sum(0), "dln_b": dy.sum(0)}
    if plant == "dW_hv_shifted":          # the text part of dW_hv one column late
        G["dW_hv"] = torch.cat([G["dW_hv"][:, :V + 1], G["dW_hv"][:, V:-1]], 1)
    B = alloc_outputs(c, tdt)
    B["out"][:n] = out
    B["d_text"][:n] = dzgv @ W_hv[:, V:] + dzga @ W_ha[:, A:] + dE
    if B["d_visual"] is not None:
        B["d_visual"][:n] = dzgv @ W_hv[:, :V] + dpv @ W_v
    if B["d_acoustic"] is not None:
        B["d_acoustic"][:n] = dzga @ W_ha[:, :A] + dpa @ W_a
    for k in GRADS:
        if (c["dw_zero"] and k.startswith("dW_")) or (plant == "bias_grad_stored" and k == "db_v"):
            B[k] = G[k].clone()
        else:
            B[k] = B[k] + G[k]
    return B, (c["path"] if c["hook"] else None)


# ------------------------------------------------------------------------------------------------------------------------ measurement
def measure_units(cases=None):
    """{(dtype, output): (largest cpu_unit, case)} over the cases"""
    worst = {}
    for c in cases or ALL_CASES:
        for _, tdt in DTS:
            for k, x in cpu_unit(c, tdt).items():
                if x > worst.get((DT_NAME[tdt], k), (-1.0, ""))[0]:
                    worst[DT_NAME[tdt], k] = (x, c["name"])
    return worst


def measure_kernel(cases=None, dev="cuda"):
    """{(dtype, output): (the kernel's largest |err| / scale, case)}; every case is checked on the way"""
    worst = {}
    for c in cases or ALL_CASES:
        for _, tdt in DTS:
            got, path = run_gpu(c, tdt, dev)
            for k, x in check(c, tdt, got, path).items():
                if x > worst.get((DT_NAME[tdt], k), (-1.0, ""))[0]:
                    worst[DT_NAME[tdt], k] = (x, c["name"])
    return worst


def _round_up(x):
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return math.ceil(x / 10 ** e) * 10 ** e


if __name__ == "__main__":
    import sys
    w = measure_units()
    print("# UNIT: largest CPU error in units of the scale (f32: float32 evaluation, bf16: storage model vs float64 oracle), case")
    for (d, k), (x, n) in sorted(w.items()):
        print('    ("%s", "%s"): %.2g,   # %.4g at %s' % (d, k, _round_up(x), x, n))
    if "--gpu" in sys.argv:
        print("# kernel: largest error in the same units, case")
        for (d, k), (x, n) in sorted(measure_kernel().items()):
            print("%-5s %-11s kernel %.4g (%.2f of 4 * UNIT) at %s" % (d, k, x, x / (ALLOW * unit(d, k)) if unit(d, k) else float("inf"), n))
