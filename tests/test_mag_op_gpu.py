"""The Multimodal Adaptation Gate at operator level (csrc/mag.hip, mag_fwd_impl / mag_bwd_impl): one forward and one backward per case against
the float64 reference of tests/mag_op_helpers.py -- row-block edges (4 rows per forward block, 8 per backward block, two per wave), one to
four 64-row k stages, the modality widths around the 64-column pad, bf16 at every hidden size, null rows inside a wave's row pair, the
contract of the C ABI, and the path the two engines take (padded text, caller-kept pad rows, slabs, stored weight gradients) through
mb_debug_mag_forward_ex / mb_debug_mag_backward_ex.  The cases, the reference and the bounds are the helpers'; this file only calls them."""
import pytest
import torch

import mag_op_helpers as M

pytestmark = pytest.mark.gpu
DTYPES = [pytest.param(tdt, id=M.DT_NAME[tdt]) for _, tdt in M.DTS]


@pytest.mark.parametrize("tdt", DTYPES)
@pytest.mark.parametrize("c", M.STANDALONE_CASES, ids=M._id)
def test_mag_operator(c, tdt):
    got, path = M.run_gpu(c, tdt)
    M.check(c, tdt, got, path)


@pytest.mark.parametrize("tdt", DTYPES)
@pytest.mark.parametrize("c", M.ENGINE_CASES, ids=M._id)
def test_mag_engine_path(c, tdt):
    got, path = M.run_gpu(c, tdt)
    M.check(c, tdt, got, path)


@pytest.mark.parametrize("tdt", DTYPES)
def test_mag_reused_workspace_is_bit_identical(tdt):
    """forward + backward at T = 65, then at T = 9 on the same workspace: within the bounds, and `out` is that of a fresh (0xFF-filled)
    workspace bit for bit"""
    reused, fresh = M.run_reused_workspace(tdt)
    it = M.CANARY[tdt][0]
    assert torch.equal(reused["out"].view(it), fresh["out"].view(it))
    assert bool(torch.isfinite(fresh["out"][:9].float()).all())


@pytest.mark.parametrize("dt", [M.F32, M.BF16])
def test_mag_refused_shapes(dt):
    """V < 1, A < 1 and hidden sizes outside 256 | 512 | 768 | 1024: MB_ERR_SHAPE from forward, backward and both hooks;
    slabs without enough scratch: MB_ERR_ARG"""
    for what, rc in M.refusals(dt):
        assert rc == M.MB_ERR_SHAPE, (what, rc)
    for what, rc in M.arg_refusals(dt):
        assert rc == M.MB_ERR_ARG, (what, rc)
