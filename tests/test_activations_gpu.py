"""GPU: the feed-forward activations next to erf-GELU -- relu, swish, gelu_new, mish -- at operator level: epilogues 7 .. 10 of mb_gemm /
mb_debug_gemm_ex (csrc/common.h relu_pair / swish_pair / gelu_new_pair / mish_pair, one epilogue mode EPI_BIAS_ACT in gemm_tile.h)
against fp64 torch on the CPU, act' from autograd in fp64.

Bounds are the ones erf-GELU's epilogue has always had: test_ops_gpu.close() x 1 for C = act'(u), x 2 for C2 = act(u), against the
dtype of the launch.  One refinement, for relu only: relu' jumps at u = 0, and the kernel's u is an fp32 sum in some order -- where the
fp64 |u| is below K 2^-24 (|A| |B|^T) (the worst case of any fp32 summation order, as in gemm_op_helpers) plus the fp32 bias add, both
sides of the jump are correct and either value is accepted; everywhere else relu' must be exactly 0 or 1 and the bound holds as it is.

What tells the activations apart is asserted on the CPU references of every fp32 case: any two of the five differ somewhere in act' by
more than 10 x the tolerance (gelu_new vs gelu: 8.7e-4 at u ~ 2 against 2.3e-5).  bf16 cannot separate gelu_new from gelu (its
tolerance is 1.2e-2) and does not try: in bf16 the kernel that ran (mb_debug_gemm_last_kernel) and the fp32 run of the same code do."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import _lib, rng
from gemm_op_helpers import (BIAS_GELU, DTS, GUARD, MB_ERR_MODE, NT, canary, case, is_canary, kernel_key, last_kernel, poisoned, predict)
from test_ops_gpu import DEV, close, stream, tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_activations import ACTS, act_fn      # noqa: E402

NEW = ("relu", "swish", "gelu_new", "mish")
EPI = {"gelu": _lib.EPI_BIAS_GELU, "relu": _lib.EPI_BIAS_RELU, "swish": _lib.EPI_BIAS_SWISH, "gelu_new": _lib.EPI_BIAS_GELU_NEW,
       "mish": _lib.EPI_BIAS_MISH}
EPI_BIAS_ACT = 7                     # the internal mode (kernels.h) every new activation runs: the MODE argument of the kernel templates

# (M, N, K, tile): every kernel form erf-GELU's epilogue has -- 64 x 64 (three-slot ring in bf16), 128 x 128, 128 x 64, the 12872 request
# that falls back to 64 x 64, 256 x 128 ping-pong (bf16; 128 x 128 in fp32), the same request with a ragged N and two k stages (which
# the ping-pong kernel does not take: 128 x 128), and the engine's own launch
FORMS = [(150, 192, 128, 64), (300, 256, 384, 128), (300, 200, 384, 12864), (130, 64, 512, 12872), (512, 256, 384, 256), (300, 136, 192, 256)]
ENGINE = (2400, 3072, 768, 0)
PAD = (8, 24, 8, 24)                 # lda, ldb, ldc, ldr over the natural ones (gemm_op_helpers.case)


def literals(sym):
    """(function name, the literal template arguments in order) of a kernel symbol, mangled or demangled (as gemm_op_helpers.kernel_key)"""
    s = sym.strip()
    if s.startswith("_ZN2mb"):
        j = 6
        while s[j].isdigit():
            j += 1
        n = int(s[6:j])
        fn, rest = s[j:j + n], s[j + n:]
        return fn, [(-int(v[1:]) if v.startswith("n") else int(v)) for v in re.findall(r"L[a-z](n?[0-9]+)E", rest.split("Ev")[0] + "E")]
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
    return fn, lits


def mode_of(sym):
    """the MODE template argument: gemm2_kernel / gemm_kernel <T, BM, BN, AK, BK, MODE, ...>, gemm_pp_kernel <AK, BK, MODE>"""
    fn, lits = literals(sym)
    return lits[2] if fn == "gemm_pp_kernel" else lits[4]


# ------------------------------------------------------------------------------------------------ references, computed once per shape
_REF = {}


def reference(M, N, K):
    """operands exact in bf16 (so in both dtypes) with u spanning at least [-6, 6]; per activation (act(u), act'(u)) in fp64, and the
    summation-order uncertainty of u"""
    if (M, N, K) in _REF:
        return _REF[(M, N, K)]
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    A = ((torch.rand((M, K), generator=g) * 2 - 1)).to(torch.bfloat16).float()
    B = ((torch.rand((N, K), generator=g) * 2 - 1) * (9.0 / K ** 0.5)).to(torch.bfloat16).float()      # std(u) ~ 3
    bias = (torch.rand((N,), generator=g) * 2 - 1)
    u = A.double() @ B.double().t() + bias.double()
    assert float(u.min()) <= -6.0 and float(u.max()) >= 6.0, (float(u.min()), float(u.max()))
    delta = K * 2.0 ** -24 * (A.abs().double() @ B.abs().double().t()) + 2.0 ** -23 * u.abs() + 1e-30
    r = dict(A=A, B=B, bias=bias, u=u, delta=delta, act={})
    for a in ACTS:
        x = u.clone().requires_grad_(True)
        y = act_fn(a)(x)
        (d,) = torch.autograd.grad(y.sum(), x)
        r["act"][a] = (y.detach(), d.detach())
    _REF[(M, N, K)] = r
    return r


def launch(dt, tdt, epi, M, N, K, r, tile=0, drop=None, layout=NT, hook=False, want_rc=0):
    """-> (C = act', C2 = act) as float64 [M][N], after checking that nothing outside them was written"""
    L = _lib.lib()
    lda, ldb, ldc = K + PAD[0], K + PAD[1], N + PAD[2]
    Ab, Bb = poisoned(r["A"], lda, GUARD, tdt).to(DEV), poisoned(r["B"], ldb, GUARD, tdt).to(DEV)
    Cb, C2b = canary((M + GUARD, ldc), tdt).to(DEV), canary((M + GUARD, ldc), tdt).to(DEV)
    bb = torch.cat([r["bias"], torch.full((8,), float("nan"))]).to(DEV)
    dk = C.byref(drop) if drop is not None else None
    if hook:
        rc = L.mb_debug_gemm_ex(dt, layout, epi, M, N, K, _lib.ptr(Ab), lda, _lib.ptr(Bb), ldb, _lib.ptr(Cb), ldc, _lib.ptr(C2b), None,
                                _lib.ptr(bb), None, 0, 1.0, dk, 1, tile, 0, 0, 0, 0, None, 0, None, None, None, None, None, 0, 0, 0,
                                0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 1.0, None, None, stream())
    else:
        rc = L.mb_gemm(dt, layout, epi, M, N, K, _lib.ptr(Ab), lda, _lib.ptr(Bb), ldb, _lib.ptr(Cb), ldc, _lib.ptr(C2b), None,
                       _lib.ptr(bb), None, 0, 1.0, dk, 1, tile, stream())
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    Cc, C2c = Cb.cpu(), C2b.cpu()
    if want_rc != 0:
        assert bool(is_canary(Cc).all()) and bool(is_canary(C2c).all())
        return None, None
    for name, buf in (("C", Cc), ("C2", C2c)):
        assert bool(is_canary(buf[M:]).all()) and bool(is_canary(buf[:M, N:]).all()), "%s: written outside [M][N]" % name
        assert not bool(is_canary(buf[:M, :N]).any()), "%s: elements left unwritten" % name
    return Cc[:M, :N].double(), C2c[:M, :N].double()


def check(name, dt, d, g, r, mask=None, what=""):
    """close() x 1 on act', x 2 on act; relu' exact, with the jump's two sides accepted where u is not decided (the file header)"""
    y, dy = r["act"][name]
    if mask is not None:
        y = y * mask
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(g).all()), what
    err_d = (d - dy).abs()
    if name == "relu":
        assert bool(((d == 0) | (d == 1)).all()), what + ": relu' is 0 or 1"
        err_d = torch.where(r["u"].abs() <= r["delta"], torch.zeros_like(err_d), err_d)
    td, tg = tol(dt, dy), 2.0 * tol(dt, y)
    ed, eg = float(err_d.max()), float((g - y).abs().max())
    print("%s %s %s: act' max|err| %.3e (tol %.3e), act max|err| %.3e (tol %.3e)" % (what, name, "fp32" if dt == _lib.DT_F32 else "bf16", ed, td, eg, tg))
    assert ed <= td, "%s %s': max|err| %.3e > tol %.3e" % (what, name, ed, td)
    assert eg <= tg, "%s %s: max|err| %.3e > tol %.3e" % (what, name, eg, tg)


def separated(r, dt):
    """precondition (fp32): any two activations differ somewhere in act' by more than 10 x the tolerance"""
    for a, b in itertools.combinations(ACTS, 2):
        da, db = r["act"][a][1], r["act"][b][1]
        gap = float((da - db).abs().max())
        assert gap > 10 * max(tol(dt, da), tol(dt, db)), (a, b, gap)


def expected_key(M, N, K, tile, tdt):
    """the kernel erf-GELU's epilogue runs for this launch (gemm_op_helpers.predict: the launchers' documented selection)"""
    return predict(case("act", NT, BIAS_GELU, M, N, K=K, tile=tile, pad=PAD), tdt)


# ------------------------------------------------------------------------------------------------ kernel forms
@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("M,N,K,tile", FORMS)
def test_every_kernel_form(dt, tdt, M, N, K, tile):
    r = reference(M, N, K)
    if dt == _lib.DT_F32:
        separated(r, dt)
    want = expected_key(M, N, K, tile, tdt)
    # erf-GELU first: the launch still runs the kernel it has always run
    launch(dt, tdt, EPI["gelu"], M, N, K, r, tile)
    sym = last_kernel()
    assert kernel_key(sym) == want and mode_of(sym) == 1, (sym, want)
    for name in NEW:
        d, g = launch(dt, tdt, EPI[name], M, N, K, r, tile)
        sym = last_kernel()
        assert kernel_key(sym) == want and mode_of(sym) == EPI_BIAS_ACT, (name, sym, want)
        check(name, dt, d, g, r, what="%dx%dx%d tile %d" % (M, N, K, tile))


def test_gelu_launches_name_the_symbols_they_always_named():
    """the engine's FFN1 launch and the 256 x 128 request, bf16, epilogue 1: the same template instantiations as before EPI_BIAS_ACT existed"""
    M, N, K, _ = ENGINE
    r = reference(M, N, K)
    launch(_lib.DT_BF16, torch.bfloat16, EPI["gelu"], M, N, K, r, 0)
    fn, lits = literals(last_kernel())
    assert (fn, lits) == ("gemm2_kernel", [128, 128, 0, 0, 1, 2, 128, 0, 4]), (fn, lits)
    launch(_lib.DT_BF16, torch.bfloat16, EPI["gelu"], M, N, K, r, 256)
    fn, lits = literals(last_kernel())
    assert (fn, lits) == ("gemm_pp_kernel", [0, 0, 1]), (fn, lits)


@pytest.mark.parametrize("name", NEW)
def test_the_engines_own_launch_bf16(name):
    """[2400 x 3072] = [2400 x 768] [3072 x 768]^T, tile 0: what both engines launch for FFN1 at the benchmark shape"""
    M, N, K, tile = ENGINE
    r = reference(M, N, K)
    d, g = launch(_lib.DT_BF16, torch.bfloat16, EPI[name], M, N, K, r, tile)
    sym = last_kernel()
    assert kernel_key(sym) == expected_key(M, N, K, tile, torch.bfloat16) == "g2:128x128:2:128" and mode_of(sym) == EPI_BIAS_ACT, sym
    check(name, _lib.DT_BF16, d, g, r, what="engine launch")


# ------------------------------------------------------------------------------------------------ bias sweep: u = bias exactly
def sweep_values():
    pm = lambda v: [v, -v]
    vals = [0.0, -0.0] + sum((pm(v) for v in (1e-6, 0.5, 1.0, 2.0, 2.7, 5.0, 10.0, 19.9, 20.1, 50.0, 88.0, 1e3, 1e4)), [])
    rest = torch.linspace(-8.0, 8.0, 192 - len(vals)).tolist()
    return torch.tensor(vals + rest, dtype=torch.float32)


@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("name", NEW)
def test_bias_sweep_saturation_and_zero(name, dt, tdt):
    """A = 0: u[m][n] = bias[n] exactly (fp32, whatever the dtype of the launch) -- both tails up to 1e4, both zeros, the clamp of mish at 20"""
    M, N, K = 16, 192, 128
    bias = sweep_values()
    u = bias.double().expand(M, N).contiguous()
    x = u.clone().requires_grad_(True)
    y = act_fn(name)(x)
    (dy,) = torch.autograd.grad(y.sum(), x)
    r = dict(A=torch.zeros(M, K), B=torch.ones(N, K), bias=bias, u=u, delta=torch.zeros_like(u), act={name: (y.detach(), dy)})
    d, g = launch(dt, tdt, EPI[name], M, N, K, r, 0)
    check(name, dt, d, g, r, what="bias sweep")       # finite, and the same bounds (relu: no undecided element, delta = 0)
    if name == "relu":
        assert bool((d[:, :2] == 0).all()), "relu' at +-0.0"
        assert bool((d == (u > 0).double()).all())
        if dt == _lib.DT_F32:
            assert bool((g[u > 0] == u[u > 0]).all()), "relu(u) = u exactly in fp32"
        assert bool((g[u <= 0] == 0).all())
    # the limits themselves, element-wise (the global bound above is relative to max |ref| = 1e4 for act)
    big = u.abs() >= 50
    lim_d = (u > 0).double()
    assert float((d - lim_d)[big].abs().max()) <= tol(dt, lim_d), "act' at |u| >= 50"
    rel = ((g - y.detach()).abs() / u.abs().clamp(min=1.0))[big]
    assert float(rel.max()) <= (2e-5 if dt == _lib.DT_F32 else 1.2e-2), "act at |u| >= 50"


# ------------------------------------------------------------------------------------------------ activation dropout (MAG-XLNet's use)
@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("name", NEW)
def test_activation_dropout_masks_act_only(name, dt, tdt):
    M, N, K, tile = FORMS[0]
    r = reference(M, N, K)
    key = _lib.make_dropkey(11, 3, 17, 0.1)
    mask = torch.from_numpy(rng.keep_mult(M * N, rng.make_key(11, 3, 17, 0.1))).view(M, N).double()
    assert 0.05 < float((mask == 0).double().mean()) < 0.15
    d, g = launch(dt, tdt, EPI[name], M, N, K, r, tile, drop=key, hook=True)
    check(name, dt, d, g, r, mask=mask, what="dropout 0.1")      # C2 = act(u) * mask, C unmasked
    assert bool((g[mask == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ forward -> EPI_DGELU
@pytest.mark.parametrize("dt,tdt", DTS)
@pytest.mark.parametrize("name", NEW)
def test_chain_into_the_dgelu_backward(name, dt, tdt):
    """epilogue 7 .. 10, then EPI_DGELU (layout 1) with R = the saved C: dX = (dY W2) o act'(u) and its column sums, the bounds of
    test_ops_gpu.test_gemm_nn_dgrad"""
    L = _lib.lib()
    M, N, K = 150, 192, 128                      # forward [M x N] from K; backward dX [M x N] = dY [M x K2] W2 [K2 x N]
    K2 = 128
    r = reference(M, N, K)
    Ad, Bd = r["A"].to(DEV, tdt).contiguous(), r["B"].to(DEV, tdt).contiguous()
    bd = r["bias"].to(DEV)
    saved, act = torch.zeros(M, N, dtype=tdt, device=DEV), torch.zeros(M, N, dtype=tdt, device=DEV)
    _lib.check(L.mb_gemm(dt, _lib.GEMM_NT, EPI[name], M, N, K, _lib.ptr(Ad), K, _lib.ptr(Bd), K, _lib.ptr(saved), N, _lib.ptr(act), None,
                         _lib.ptr(bd), None, 0, 1.0, None, 1, 0, stream()))
    g = torch.Generator().manual_seed(77)
    dY = (torch.rand((M, K2), generator=g) * 2 - 1).to(tdt).float()
    W2 = ((torch.rand((K2, N), generator=g) * 2 - 1) * 0.1).to(tdt).float()
    dX = torch.zeros(M, N, dtype=tdt, device=DEV)
    cs = torch.zeros(N, dtype=torch.float32, device=DEV)
    dYd, W2d = dY.to(DEV, tdt).contiguous(), W2.to(DEV, tdt).contiguous()
    _lib.check(L.mb_gemm(dt, _lib.GEMM_NN, _lib.EPI_DGELU, M, N, K2, _lib.ptr(dYd), K2, _lib.ptr(W2d), N, _lib.ptr(dX), N, None, _lib.ptr(cs),
                         None, _lib.ptr(saved), N, 1.0, None, 1, 0, stream()))
    torch.cuda.synchronize()
    ref = (dY.double() @ W2.double()) * r["act"][name][1]
    got = dX.float().cpu().double()
    if name == "relu":                           # an undecided gate (file header) would move its element by the whole product: none here
        assert not bool((r["u"].abs() <= r["delta"]).any())
    close(got, ref, dt, "%s chain dX" % name)
    close(cs.cpu().double(), ref.sum(0), dt, "%s chain column sums" % name)


# ------------------------------------------------------------------------------------------------ refused
@pytest.mark.parametrize("layout", [_lib.GEMM_NN, _lib.GEMM_TN])
@pytest.mark.parametrize("name", NEW)
def test_other_layouts_are_refused(name, layout):
    M, N, K = 128, 128, 128
    g = torch.Generator().manual_seed(5)
    r = dict(A=torch.rand((M, K), generator=g), B=torch.rand((N, K), generator=g), bias=torch.zeros(N))
    for hook in (False, True):
        launch(_lib.DT_BF16, torch.bfloat16, EPI[name], M, N, K, r, 0, layout=layout, hook=hook, want_rc=MB_ERR_MODE)
    launch(_lib.DT_BF16, torch.bfloat16, 11, M, N, K, r, 0, want_rc=MB_ERR_MODE)        # the first code behind the table
