"""The MAG operator suite's own checks, without a GPU (tests/mag_op_helpers.py): the reference and its storage model, the unit constants, the
1 % cap on rows left out, and the checker itself -- it must accept a float32 stand-in of the operator in every case and reject the
stand-in with each of ten planted errors in at least one."""
import pytest
import torch

import mag_op_helpers as M

F32 = torch.float32
BY_NAME = {c["name"]: c for c in M.ALL_CASES}
# where each planted error shows (any one case is enough; the first is the one it was planted for)
PLANT_CASES = {
    "thr_eps_1e-5": ["null_beta0.001_p0", "beta1e-3"],          # the faint modality row: hm_norm ~ 1e-3, thr < 1
    "no_hm_replacement": ["null_beta0.001_p0", "null_beta1_p0.5"],
    "no_clamp": ["T65", "beta64"],
    "no_dnorm_e": ["T65", "beta1e-3"],
    "gate_ge": ["null_beta1_p0", "null_H1024"],                  # the gate columns whose pre-activation is exactly zero
    "ln_eps_1e-12": ["T65", "null_beta1_p0"],
    "no_dropout_bwd": ["T65", "p0.1"],
    "last_row_dropped": ["T65", "T1", "T9"],
    "dW_hv_shifted": ["T65", "V64_A128", "V1_A1"],
    "bias_grad_stored": ["g0", "eng_T65_V47_A74_dz0"],
}


def test_case_lists_cover_the_issue():
    names = set(BY_NAME)
    assert len(names) == len(M.ALL_CASES)
    assert all(c["T"] <= 193 for c in M.ALL_CASES)
    assert {c["T"] for c in M.STANDALONE_CASES} >= {1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129, 193}
    assert {(c["H"], c["T"]) for c in M.STANDALONE_CASES} >= {(H, T) for H in (256, 512, 768, 1024) for T in (9, 65)}
    assert {(c["V"], c["A"]) for c in M.STANDALONE_CASES} >= set(M.VA_LIST)
    eng = [c for c in M.ENGINE_CASES if c["text_padded"]]
    assert all(c["pads_clean"] and c["slabs"] and c["path"] == (1, 1, 64) for c in eng)
    for dz in (0, 1):
        assert {(c["T"], c["V"], c["A"]) for c in eng if c["dw_zero"] == dz and c["H"] == 768} == \
            {(T, V, A) for T in (1, 9, 64, 65, 129, 193) for V, A in M.VA_LIST}
        assert {c["H"] for c in eng if c["dw_zero"] == dz} == {256, 768, 1024}
    hm0, e0, faint = M.null_rows(21)
    kinds = {(a in hm0 or a in e0, b in hm0 or b in e0) for a, b in zip(range(0, 20, 2), range(1, 21, 2))}
    assert kinds == {(True, False), (False, True), (True, True), (False, False)} and 20 in hm0 and set(hm0) & set(e0)


@pytest.mark.parametrize("name", ["T9", "null_beta1_p0.5", "V65_A129", "beta1e-3"])
def test_restatement_is_the_oracle(name):
    """graph() (which supplies the scales and, with storage on, the bf16 reference) against oracle.mag_bert_ref.MAG itself, float64"""
    c = BY_NAME[name]
    R = M.reference(c, F32)              # (its `ref` is the oracle's result)
    got, _ = M.evaluate(R["I"], c["beta"], False, torch.float64, R["I"]["keep"])
    for k in M.OUTPUTS:
        assert float((got[k] - R["ref"][k]).abs().max()) <= 1e-11 * max(1.0, float(R["ref"][k].abs().max())), k


@pytest.mark.parametrize("c", M.ALL_CASES, ids=M._id)
def test_reference_units_cap_and_standin(c):
    """per case: finite reference, at most 1 % of the rows left out, the clamp on the sides the case is about, and the checker accepts the float32 stand-in"""
    for _, tdt in M.DTS:
        R = M.reference(c, tdt)
        assert R["fragile"] <= M.CAP * c["T"], (M.DT_NAME[tdt], R["fragile"])
        for k in M.OUTPUTS:
            assert bool(torch.isfinite(R["ref"][k]).all()), k
        thr = R["thr"]
        if c["beta"] == 1e-3:
            assert bool((thr < 1).all())
        elif c["beta"] == 64.0:
            assert bool((thr[R["I"]["text"].float().abs().amax(-1) > 0] > 1).all())
        elif c["T"] >= 4:
            assert bool((thr < 1).any()) and bool((thr > 1).any())
    got, path = M.run_model(c, F32)
    M.check(c, F32, got, path)


def test_units_are_the_measured_maxima():
    """UNIT is what the CPU gives, not a guess.  bf16: the storage model against the oracle, both float64 -- the largest value over the
    cases lies within 10 % below the committed constant.  fp32: a float32 matmul sums in the order its BLAS picks for the machine and the
    thread count (two machines gave 2.3e-8 and 4.5e-8 for d_visual, the widest gap of the fourteen): within a factor 2.5 either way."""
    worst = M.measure_units()
    for (d, k), u in M.UNIT.items():
        w = worst[d, k][0]
        if d == "bf16":
            assert u * 0.9 <= w <= u, (d, k, worst[d, k], u)
        else:
            assert u / 2.5 <= w <= u * 2.5, (d, k, worst[d, k], u)


@pytest.mark.parametrize("plant", M.PLANTS)
def test_planted_error_is_caught(plant):
    caught = []
    for name in PLANT_CASES[plant]:
        c = BY_NAME[name]
        got, path = M.run_model(c, F32, plant)
        try:
            M.check(c, F32, got, path)
        except AssertionError as e:
            caught.append((name, str(e)[:200]))
    assert caught, "no case of %r notices %s" % (PLANT_CASES[plant], plant)
    assert caught[0][0] == PLANT_CASES[plant][0], caught


def test_wrong_path_is_caught():
    c = BY_NAME["eng_T65_V47_A74_dz1"]
    got, _ = M.run_model(c, F32)
    with pytest.raises(AssertionError, match="path"):
        M.check(c, F32, got, (0, 0, 64))
    for T in (1, 64, 65):
        for _, tdt in M.DTS:
            assert M.path_table(tdt, T, 1) == (1, 1, 64) and M.path_table(tdt, T, 0) == (0, 0, 64)


def test_workspace_layout_mirror():
    """ws_layout() restates MagWs::init; with a library at hand the byte count must agree"""
    from bert_multimodal_transformer_amd import _lib
    L = _lib.lib()
    for dt in (M.F32, M.BF16):
        for T, H, V, A in ((1, 256, 1, 1), (65, 768, 47, 74), (193, 1024, 65, 129), (64, 512, 64, 128)):
            assert M.ws_layout(dt, T, H, V, A)[1] == L.mb_mag_workspace_bytes(dt, T, H, V, A)
            assert L.mb_debug_mag_slab_bytes(T, H) == 2 * ((T + 7) // 8) * 3 * H * 4


@pytest.mark.parametrize("dt", [M.F32, M.BF16])
def test_refusals_come_before_any_launch(dt):
    """shapes the operator does not take and slabs without scratch are refused on the host, before a pointer is read: no GPU needed"""
    for what, rc in M.refusals(dt):
        assert rc == M.MB_ERR_SHAPE, (what, rc)
    for what, rc in M.arg_refusals(dt):
        assert rc == M.MB_ERR_ARG, (what, rc)
