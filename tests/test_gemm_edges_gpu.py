"""GPU: the GEMM family (csrc/gemm.hip, gemm_pp.hip, gemm_tile.h) at operator level against fp64 restatements of the same formulas, at the
stage counts next to every k loop's prologue and peeled tail, at the row and column edges of every tile, with non-natural leading
dimensions, NaN around every operand and a canary around every output, and with what mb_gemm cannot reach: segmented B, cvalid,
overwrite, deterministic column sums, the deeper rings of the grouped launch and every rider host.  Every case asserts which kernel ran
(mb_debug_gemm_last_kernel), the documented fallbacks included.  Machinery, bounds and the case lists: tests/gemm_op_helpers.py; the
same checks against a CPU stand-in with planted errors: tests/test_gemm_edges_cpu.py.

Both dtypes run every case: a kernel that does not exist in fp32 (the ping-pong kernels, the dgrad rider hosts) is asserted as the
fallback or the refusal the launchers document, never skipped.  SKIPS_EXPECTED states that and the last test asserts it.

Measured on the MI355X (profiles/gemm_edge_errors.txt has the table per family, dtype and epilogue; 853 cases in 6 s): worst |err| /
bound 0.993 for bf16 T outputs (the bound is the half-ulp of the one output rounding: an element just above a binade edge sits at it; the
CPU stand-in reaches the same 0.993), at most 0.12 for fp32 T / fp32 outputs and 0.22 for column sums.  EPI_BIAS_GELU against fp64, worst
|err| over all cases (and as a share of its close() ceiling): gelu' 3.906e-3 (0.29) in bf16, 7.9e-7 (0.033) in fp32; gelu 9.45e-3 (0.14)
in bf16, 1.37e-6 (0.012) in fp32."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_op_helpers as H
from bert_multimodal_transformer_amd import _lib
from gemm_op_helpers import ADD_RES, BF16, DGELU, F32, NN

DEV = "cuda:0"
CASES = H.single_cases()
SKIPS_EXPECTED = 0           # cases of this file that may skip: none
_ran = {"edge": 0, "rider": 0}
_report = {}


def _note(fam, tdt, epi, name, ratio, err):
    k = (fam, str(tdt).replace("torch.", ""), H.EPI_NAMES[epi], name)
    r = _report.get(k, (0.0, 0.0))
    _report[k] = (max(r[0], ratio), max(r[1], err))


def _expect_kernel(c, dt, tdt, sym, what):
    key, want = H.kernel_key(sym), H.predict(c, tdt)
    print("%s %s: tile %d -> %s (%s)" % (what, tdt, c["tile"], key, sym))
    assert key == want, "%s: ran %s, the documented selection is %s" % (what, key, want)
    if dt == BF16:
        assert key.startswith(c["want"]), "%s: ran %s, the case is about %s" % (what, key, c["want"])
    elif c["want_f32"] is not None:
        assert key == c["want_f32"], "%s: ran %s, the case is about %s" % (what, key, c["want_f32"])


@pytest.mark.parametrize("dt,tdt", H.DTS)
@pytest.mark.parametrize("c", CASES, ids=[H.case_id(c) for c in CASES])
def test_gemm_edge_case(dt, tdt, c):
    what = H.case_id(c)
    p = H.problem(c, tdt)
    rc, outs, sym, _ = H.run_gpu(c, dt, tdt, p, DEV)
    assert rc == 0, "%s: %s" % (what, _lib.lib().mb_error_string(rc).decode())
    print("%s %s: tile %d -> %s" % (what, tdt, c["tile"], H.kernel_key(sym)))
    res = H.check(c, tdt, p, outs, what=what)             # (numbers first: a wrong kernel with right numbers and a right kernel with wrong ones read differently)
    for name, (ratio, err) in res.items():
        print("%s %s %s: worst |err| / bound %.3f, max |err| %.3e" % (what, tdt, name, ratio, err))
        _note(c["name"], tdt, c["epi"], name, ratio, err)
    _expect_kernel(c, dt, tdt, sym, what)
    _ran["edge"] += 1


@pytest.mark.parametrize("dt,tdt", H.DTS)
@pytest.mark.parametrize("c", H.REFUSAL_CASES, ids=[H.case_id(c) for c in H.REFUSAL_CASES])
def test_segmented_b_refusals(dt, tdt, c):
    """refused by the launcher, before any launch: MB_ERR_SHAPE and an untouched output"""
    p = H.problem(c, tdt)
    rc, outs, _, _ = H.run_gpu(c, dt, tdt, p, DEV)
    assert rc == H.MB_ERR_SHAPE, (H.case_id(c), rc)
    assert bool(H.is_canary(outs["C"]).all())


# ------------------------------------------------------------------------------------------------ grouped launch: cvalid, overwrite, rings
def _grouped_want(dt, tile, stages, K):
    nt = K // (64 if dt == BF16 else 32)
    if stages in (4, 5) and tile == 64:
        return "g2grp:64x64:%d:128" % stages
    return "g2grp:%dx%d:%d:128" % (tile, tile, 3 if (dt == BF16 and nt < 2) else 2)


@pytest.mark.parametrize("dt,tdt", H.DTS)
@pytest.mark.parametrize("overwrite", [0, 1])
@pytest.mark.parametrize("K", H.GROUPED_K)
@pytest.mark.parametrize("tile,stages,Vp", H.GROUPED)
def test_grouped_cvalid(dt, tdt, tile, stages, Vp, K, overwrite):
    """MAG's six problems at H = 128, V = 47, A = 74: column ranges of shared tensors 178 / 205 / 50 / 77 floats wide from 4-byte-aligned bases"""
    what = "grouped tile %d stages %d K %d overwrite %d %s" % (tile, stages, K, overwrite, tdt)
    g = H.grouped_problem(tdt, K, Vp=Vp, overwrite=overwrite)
    rc, outs, sym = H.grouped_run_gpu(dt, g, tile, stages, DEV)
    assert rc == 0, "%s: %s" % (what, _lib.lib().mb_error_string(rc).decode())
    key = H.kernel_key(sym)
    print("%s -> %s (%s)" % (what, key, sym))
    assert key == _grouped_want(dt, tile, stages, K), what
    res = H.grouped_check(g, outs, what=what)
    for o, (ratio, err) in res.items():
        print("%s dW_%s: worst |err| / bound %.3f, max |err| %.3e" % (what, o, ratio, err))
        _note("grouped%d/%d" % (tile, stages), tdt, H.ACCUM_F32, "cvalid" + ("=" if overwrite else "+="), ratio, err)


@pytest.mark.parametrize("dt,tdt", H.DTS)
def test_grouped_refusals(dt, tdt):
    g = H.grouped_problem(tdt, 128, overwrite=1)
    cv = [p[7] for p in g["probs"]]
    rc, outs, _ = H.grouped_run_gpu(dt, g, 64, 0, DEV, cvalid=[cv[0] + 1] + cv[1:])          # cvalid > N
    assert rc == H.MB_ERR_SHAPE and all(bool(H.is_canary(t).all()) for t in outs.values())
    ragged = [(100,) + g["probs"][0][1:]] + g["probs"][1:]                                    # M is no whole tile
    rc, outs, _ = H.grouped_run_gpu(dt, g, 64, 0, DEV, probs=ragged)
    assert rc == H.MB_ERR_SHAPE and all(bool(H.is_canary(t).all()) for t in outs.values())
    rc, _, _ = H.grouped_run_gpu(dt, g, 64, 3, DEV)                                           # the hook takes stages 0 | 4 | 5
    assert rc == H.MB_ERR_ARG


# ------------------------------------------------------------------------------------------------ riders
_host_cache = {}


def _host(host, tdt):
    """the host's problem, its fp64 reference and the bits of the same launch without riders: once per host"""
    if (host, tdt) in _host_cache:
        return _host_cache[(host, tdt)]
    h = H.RIDE_HOSTS[host]
    dt = BF16 if tdt == torch.bfloat16 else F32
    if h["kind"] == "nn":
        c = H.case("ride-" + host, NN, h["epi"], h["M"], h["N"], K=h["K"], tile=0, drop=0.1 if h["epi"] == DGELU else 0.0)
        p = H.problem(c, tdt)
        rc, outs, sym, _ = H.run_gpu(c, dt, tdt, p, DEV)
        assert rc == 0
        H.check(c, tdt, p, outs, what=host + " without riders")
        got = (c, p, outs, H.kernel_key(sym))
    else:
        shapes = [(256, 128), (512, 128)] if h["tile"] == 256 else [(128, 128), (256, 128)]
        g = H.grouped_plain(tdt, h["K"], shapes)
        rc, outs, sym = H.grouped_run_gpu(dt, g, h["tile"], 0, DEV, cvalid=[0] * len(shapes))
        assert rc == 0
        H.grouped_check(g, outs, what=host + " without riders")
        got = (None, g, outs, H.kernel_key(sym))
    _host_cache[(host, tdt)] = got
    return got


def _ride_launch(host, dt, tdt, st):
    h = H.RIDE_HOSTS[host]
    c, p, _, _ = _host(host, tdt)
    if h["kind"] == "nn":
        rc, outs, sym, tiles = H.run_gpu(c, dt, tdt, p, DEV, ride=st)
        return rc, outs, sym, tiles
    rc, outs, sym = H.grouped_run_gpu(dt, p, h["tile"], 0, DEV, ride=st, cvalid=[0] * len(p["probs"]))
    return rc, outs, sym, -1


@pytest.mark.parametrize("zero_grad,shadow", [(0, False), (1, False), (0, True), (1, True)])
@pytest.mark.parametrize("n4i", [0, 1, 2])
@pytest.mark.parametrize("host", list(H.RIDE_HOSTS))
def test_rider_hosts(host, n4i, zero_grad, shadow):
    """bf16 (the dgrad hosts and the ping-pong group exist in bf16 only; their fp32 refusals: test_rider_refusals).  C keeps the bits of
    the launch without riders and passes the fp64 check; p / m / v / shadow / g have mb_adamw_step's bits; nothing behind 4 * n4 moves."""
    dt, tdt = BF16, torch.bfloat16
    h = H.RIDE_HOSTS[host]
    n4 = H.ride_n4s(host)[n4i]
    what = "rider %s n4 %d zero_grad %d shadow %d" % (host, n4, zero_grad, shadow)
    c, p, plain, plain_key = _host(host, tdt)
    st = H.ride_state(n4, H.RIDE_BLOCKS, zero_grad, shadow, DEV, seed=n4 + zero_grad)
    exp = H.ride_expected(st)
    rc, outs, sym, tiles = _ride_launch(host, dt, tdt, st)
    assert rc == 0, "%s: %s" % (what, _lib.lib().mb_error_string(rc).decode())
    key = H.kernel_key(sym)
    print("%s -> %s (%s), %d tiles; without riders %s" % (what, key, sym, tiles, plain_key))
    assert key == h["want"], what
    if h["kind"] == "nn":
        assert tiles > 0 and tiles % 8 == 0
        H.check(c, tdt, p, outs, what=what)
    else:
        H.grouped_check(p, outs, what=what)
    for name in plain:
        if name == "colsum":                              # (fp32 atomics: the arrival order is free)
            continue
        it = H.CANARY[plain[name].dtype][0]
        assert torch.equal(outs[name].view(it), plain[name].view(it)), "%s: %s differs from the launch without riders" % (what, name)
    H.ride_check(st, exp, what)
    _ran["rider"] += 1


def test_rider_refusals():
    tdt = torch.bfloat16
    c, p, _, _ = _host("g2-64", tdt)
    st = H.ride_state(16, 12, 1, False, DEV)              # blocks is no multiple of 8
    before = H.ride_clone(st)
    rc, outs, _, _ = H.run_gpu(c, BF16, tdt, p, DEV, ride=st)
    assert rc == H.MB_ERR_MODE and bool(H.is_canary(outs["C"]).all())
    st8 = H.ride_state(16, 8, 1, False, DEV)
    c2 = H.case("ride-none", NN, ADD_RES, 65, 200, K=128, tile=0)          # a v1 launch carries none
    p2 = H.problem(c2, tdt)
    rc, outs, _, tiles = H.run_gpu(c2, BF16, tdt, p2, DEV, ride=st8)
    assert rc == H.MB_ERR_MODE and tiles == 0 and bool(H.is_canary(outs["C"]).all())
    pf = H.problem(c, torch.float32)                      # the dgrad hosts are bf16 kernels
    rc, outs, _, tiles = H.run_gpu(c, F32, torch.float32, pf, DEV, ride=st8)
    assert rc == H.MB_ERR_MODE and tiles == 0 and bool(H.is_canary(outs["C"]).all())
    g = H.grouped_plain(tdt, 128, [(128, 128), (256, 128)])
    rc, outs, _ = H.grouped_run_gpu(BF16, g, 128, 0, DEV, ride=st, cvalid=[0, 0])            # 12 blocks
    assert rc == H.MB_ERR_ARG
    rc, outs, _ = H.grouped_run_gpu(BF16, g, 64, 0, DEV, ride=st8, cvalid=[0, 0])            # the 64 x 64 group carries none
    assert rc == H.MB_ERR_ARG
    gf = H.grouped_plain(torch.float32, 192, [(256, 128), (512, 128)])
    rc, outs, _ = H.grouped_run_gpu(F32, gf, 256, 0, DEV, ride=st8, cvalid=[0, 0])           # the ping-pong group is a bf16 kernel
    assert rc == H.MB_ERR_SHAPE
    for s, b in ((st, before),):
        for k in ("p", "g", "m", "v"):
            assert torch.equal(s[k].view(torch.int32), b[k].view(torch.int32))


def test_grouped_rider_fp32_128():
    """the 128 x 128 group is the one rider host that exists in fp32"""
    tdt = torch.float32
    g = H.grouped_plain(tdt, 64, [(128, 128), (256, 128)])
    rc, plain, _ = H.grouped_run_gpu(F32, g, 128, 0, DEV, cvalid=[0, 0])
    assert rc == 0
    n4 = H.ride_n4s("grp-128")[2]
    st = H.ride_state(n4, H.RIDE_BLOCKS, 1, True, DEV)
    exp = H.ride_expected(st)
    rc, outs, sym = H.grouped_run_gpu(F32, g, 128, 0, DEV, ride=st, cvalid=[0, 0])
    assert rc == 0 and H.kernel_key(sym) == "g2grp:128x128:2:128", sym
    H.grouped_check(g, outs, what="fp32 group with riders")
    for name in plain:
        assert torch.equal(outs[name].view(torch.int32), plain[name].view(torch.int32))
    H.ride_check(st, exp, "fp32 group")


def test_zz_report_and_no_unexpected_skips():
    """prints the table profiles/gemm_edge_errors.txt records; when the file ran as a whole, every case of the lists ran to its end in both
    dtypes -- none skipped, none left out"""
    for k in sorted(_report):
        print("REPORT %-12s %-8s %-13s %-8s worst |err| / bound %.3f  max |err| %.3e" % (k + _report[k]))
    assert SKIPS_EXPECTED == 0
    if _ran["edge"] or _ran["rider"]:                     # (alone, this test has nothing to count)
        assert _ran["edge"] == 2 * len(CASES) - SKIPS_EXPECTED, _ran
        assert _ran["rider"] == len(H.RIDE_HOSTS) * 3 * 4, _ran
