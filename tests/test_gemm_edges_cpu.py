"""CPU: the machinery of tests/test_gemm_edges_gpu.py (tests/gemm_op_helpers.py) checked against itself.  The "kernel" is an fp32 matmul
on the CPU, rounded to the compute dtype and written into the same poisoned layout the GPU kernels write into.  It must pass every bound
for every case of the lists, and each of a handful of planted errors -- the kind a subtly wrong kernel makes -- must fail: this is the
evidence that the GPU tests would notice."""
import pytest
import torch

import gemm_op_helpers as H
from gemm_op_helpers import ACCUM_F32, ADD_RES, BIAS, DGELU, NN, NT, TN

CASES = H.single_cases()
IDS = [H.case_id(c) for c in CASES]


def test_case_lists_are_what_the_issue_asks_for():
    """every family with its stage counts, both dtypes; unique ids; the selection twin names the kernel each case is about"""
    assert len(set(IDS)) == len(IDS), [i for i in IDS if IDS.count(i) > 1]
    for fam, f in H.FAMILIES.items():
        got = sorted({c["nt"] for c in CASES if c["name"] == fam})
        assert got == sorted(f["nts"]), (fam, got)
    assert sorted({c["nt"] for c in CASES if c["name"] == "p64"}) == [2, 3, 4, 5]
    assert {c["splits"] for c in CASES if c["name"] == "splitk"} == {2, 3, 8}
    assert {c["bseg"] for c in CASES if c["name"] == "seg"} == {128, 256}
    assert {c["M"] for c in CASES if c["name"] == "pp256"} >= set(H.SEAM_M) | {255, 256, 257}
    for c in CASES:
        bf = H.predict(c, torch.bfloat16)
        assert isinstance(bf, str) and bf.startswith(c["want"]), (H.case_id(c), bf, c["want"])
        f32 = H.predict(c, torch.float32)
        assert isinstance(f32, str) and (c["want_f32"] is None or f32 == c["want_f32"]), (H.case_id(c), f32)
        assert not f32.startswith(("pp:", "pn:", "pt:")), "the ping-pong kernels are bf16 kernels"
    for c in H.REFUSAL_CASES:
        for _, tdt in H.DTS:
            assert H.predict(c, tdt) == c["rc"] == H.MB_ERR_SHAPE, H.case_id(c)


def test_kernel_key_reads_mangled_and_demangled_symbols():
    k = H.kernel_key
    assert k("_ZN2mb12gemm2_kernelIDF16bLi128ELi64ELb0ELb1ELi4ELi4ELi64ELb0ELi4EEEvNS_8GemmArgsE") == "g2:128x64:4:64"
    assert k("_ZN2mb12gemm2_kernelIfLi64ELi64ELb0ELb0ELi0ELi2ELi128ELb0ELi4EEEvNS_8GemmArgsE") == "g2:64x64:2:128"
    assert k("void mb::gemm2_kernel<__bf16, 64, 64, false, false, 0, 3, 128, false, 4>(mb::GemmArgs)") == "g2:64x64:3:128"
    assert k("_ZN2mb11gemm_kernelIfLi64ELi64ELb1ELb1ELi5EEEvNS_8GemmArgsE") == "v1:64x64:2:128"
    assert k("_ZN2mb14gemm_pn_kernelILb0ELb0ELi2EEEvNS_8GemmArgsE") == "pn:128x64:3:256"
    assert k("void mb::gemm_pp_kernel<false, false, 1>(mb::GemmArgs)") == "pp:256x128:3:128"
    assert k("_ZN2mb19gemm_pt_ride_kernelENS_8GemmArgsENS_8AdamRideE") == "ptride:256x64:3:128"
    assert k("_ZN2mb17gemm2_ride_kernelIDF16bLi64ELi64ELb0ELb1ELi3ELi3ELi128EEEvNS_8GemmArgsENS_8AdamRideE") == "g2ride:64x64:3:128"
    assert k("_ZN2mb23gemm2_grouped_tn_kernelIDF16bLi64ELi64ELi5ELi128EEEvNS_15GroupedGemmArgsE") == "g2grp:64x64:5:128"
    assert k("_ZN2mb25gemm_pp_grouped_tn_kernelENS_15GroupedGemmArgsE") == "ppgrp:256x128:3:128"


@pytest.mark.parametrize("dt,tdt", H.DTS)
def test_stand_in_passes_every_bound_of_every_case(dt, tdt):
    worst = {}
    for c in CASES:
        p = H.problem(c, tdt)
        res = H.check(c, tdt, p, H.run_model(c, tdt, p), what=H.case_id(c))
        for name, (ratio, _) in res.items():
            key = (c["name"], name)
            worst[key] = max(worst.get(key, 0.0), ratio)
    for key in sorted(worst):
        print("stand-in %s %-8s %-7s worst |err| / bound %.3f" % (tdt, key[0], key[1], worst[key]))


def _pick(pred):
    got = [c for c in CASES if pred(c)]
    assert got
    return got[0]


# planted error -> a case it applies to (ragged M for the row errors; more than one tile for the shifted one; a segmented B for the last)
PLANTED = [
    ("drop_k_row", lambda c: c["name"] == "r64" and c["layout"] == NT and c["epi"] == BIAS and c["nt"] == 7),
    ("drop_k_row", lambda c: c["name"] == "pn" and c["layout"] == NN and c["epi"] == ADD_RES and c["nt"] == 7),
    ("drop_k_row", lambda c: c["name"] == "r64" and c["layout"] == TN and c["nt"] == 7),
    ("drop_k_row", lambda c: c["name"] == "t128" and c["layout"] == NN and c["epi"] == DGELU and c["nt"] == 5),
    ("last_row_above", lambda c: c["name"] == "r64" and c["layout"] == NT and c["epi"] == BIAS and c["M"] == 65 and c["nt"] == 2),
    ("last_row_above", lambda c: c["name"] == "pp256" and c["layout"] == NN and c["M"] == 257),
    ("shift_tile_cols", lambda c: c["name"] == "r64" and c["layout"] == NT and c["epi"] == ADD_RES and c["N"] == 200),
    ("shift_tile_cols", lambda c: c["name"] == "t128" and c["layout"] == TN and c["nt"] == 3),
    ("store_col_N", lambda c: c["name"] == "r64" and c["layout"] == NT and c["epi"] == BIAS),
    ("store_col_N", lambda c: c["name"] == "epi" and c["layout"] == TN and c["cvalid"] == 47 and c["overwrite"] == 1),
    ("store_row_M", lambda c: c["name"] == "pt" and c["layout"] == NT and c["epi"] == BIAS),
    ("store_row_M", lambda c: c["name"] == "r64" and c["layout"] == TN),
    ("seg_natural", lambda c: c["name"] == "seg" and c["layout"] == NN),
    ("seg_natural", lambda c: c["name"] == "seg" and c["layout"] == NT),
]


@pytest.mark.parametrize("dt,tdt", H.DTS)
@pytest.mark.parametrize("plant,pred", PLANTED, ids=["%s-%d" % (p, i) for i, (p, _) in enumerate(PLANTED)])
def test_planted_errors_fail(dt, tdt, plant, pred):
    c = _pick(pred)
    p = H.problem(c, tdt)
    H.check(c, tdt, p, H.run_model(c, tdt, p), what=H.case_id(c))                 # sound without the error
    with pytest.raises(AssertionError) as e:
        H.check(c, tdt, p, H.run_model(c, tdt, p, plant=plant), what=H.case_id(c))
    print("planted %s in %s (%s): %s" % (plant, H.case_id(c), tdt, str(e.value).splitlines()[0]))


def test_global_bound_alone_misses_a_dropped_k_element_in_bf16():
    """the reason for the element-wise bound: test_ops_gpu.close() (1.2e-2 * max|ref|) passes a bf16 result with one k element left out of
    one row, the derived bound does not"""
    c = _pick(lambda c: c["name"] == "r64" and c["layout"] == NT and c["epi"] == BIAS and c["nt"] == 7)
    tdt = torch.bfloat16
    p = H.problem(c, tdt)
    outs = H.run_model(c, tdt, p, plant="drop_k_row")
    r = H.reference(c, tdt, p)["C"][0]
    err = (outs["C"][:c["M"], :c["N"]].double() - r).abs()
    assert float(err.max()) <= H.close_tol(H.BF16, r)
    with pytest.raises(AssertionError):
        H.check(c, tdt, p, outs)


@pytest.mark.parametrize("dt,tdt", H.DTS)
@pytest.mark.parametrize("overwrite", [0, 1])
def test_grouped_stand_in_and_planted_cvalid_overrun(dt, tdt, overwrite):
    for K in H.GROUPED_K:
        g = H.grouped_problem(tdt, K, overwrite=overwrite)
        res = H.grouped_check(g, H.grouped_model(g), what="K=%d" % K)
        print("grouped stand-in %s K=%d overwrite=%d:" % (tdt, K, overwrite), {o: "%.3f" % r for o, (r, _) in res.items()})
        with pytest.raises(AssertionError):
            H.grouped_check(g, H.grouped_model(g, plant="cvalid_overrun"))


def test_rider_quad_counts_cross_a_double_half_iteration():
    for host, h in H.RIDE_HOSTS.items():
        n4s = H.ride_n4s(host)
        assert n4s[0] == 1 and n4s[1] == H.RIDE_BLOCKS - 1 and H.RIDE_BLOCKS % 8 == 0
        per_block = -(-n4s[2] // H.RIDE_BLOCKS)
        assert per_block > 2 * h["nthreads"] * h["unr"], host
