"""CPU: gradient-norm clipping, host side -- the optimizer option and what flat_step_args hands to the single-call step, the driver's
flag, the new symbols of the C ABI, and the engines' host-only checks (no device needed)."""
import ctypes as C
import os
import re

import pytest
import torch

from bert_multimodal_transformer_amd import AdamW, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mb_grad_clip_scratch_bytes", "mb_grad_clip_coef", "mb_bert_set_grad_clip", "mb_bert_grad_clip_stats",
               "mb_xlnet_set_grad_clip", "mb_xlnet_grad_clip_stats"]


class FakeCore(object):
    """what AdamW looks at of a model's flat buffer: a decay slab [0, 128) and a no-decay slab [128, 192)"""

    def __init__(self):
        self.params = torch.zeros(192)
        self.grads = torch.zeros(192)
        self.n_params = self.n_update_end = 192
        self.n_decay = 128
        self.sh_begin, self.sh_end = 0, 128
        self.tensors = [("w.weight", 0, 128, (128,), 1), ("w.bias", 128, 64, (64,), 0)]


def two_groups(core, **kw):
    w = torch.nn.Parameter(core.params[0:128])
    b = torch.nn.Parameter(core.params[128:192])
    w._mb_flat = (core, 0, 128, (128,))
    b._mb_flat = (core, 128, 64, (64,))
    return AdamW([{"params": [w], "weight_decay": 0.01}, {"params": [b], "weight_decay": 0.0}], lr=1e-3, **kw)


def test_flat_step_args_carries_max_grad_norm():
    core = FakeCore()
    assert two_groups(core).flat_step_args(core)["max_grad_norm"] == 0.0
    opt = two_groups(core, max_grad_norm=1.5)
    assert opt.max_grad_norm == 1.5 and opt.flat_step_args(core)["max_grad_norm"] == 1.5
    opt.max_grad_norm = 0.25                                     # the attribute may be changed between steps
    assert opt.flat_step_args(core)["max_grad_norm"] == 0.25
    for off in (None, 0.0, -1.0, float("inf"), float("nan")):    # everything the engine would take for "off" is 0.0
        opt.max_grad_norm = off
        assert opt.flat_step_args(core)["max_grad_norm"] == 0.0
    assert opt.last_grad_norm is None
    # a classed optimizer (one group over everything: a map of one segment) carries it too
    w = torch.nn.Parameter(core.params[0:128]); b = torch.nn.Parameter(core.params[128:192])
    w._mb_flat = (core, 0, 128, (128,)); b._mb_flat = (core, 128, 64, (64,))
    classed = AdamW([{"params": [w, b], "weight_decay": 0.01}], lr=1e-3, max_grad_norm=2.0)
    args = classed.flat_step_args(core)
    assert "map" in args and args["max_grad_norm"] == 2.0


def test_flat_step_args_declines_the_data_parallel_single_call_when_clipping():
    core = FakeCore()
    plain, clip = two_groups(core), two_groups(core, max_grad_norm=1.0)
    plain._dp = clip._dp = object()
    assert plain.flat_step_args(core, allow_dp=True) is not None
    assert clip.flat_step_args(core, allow_dp=True) is None and clip.flat_step_args(core) is None
    clip.max_grad_norm = None
    assert clip.flat_step_args(core, allow_dp=True) is not None


def test_driver_flag_and_default():
    from bert_multimodal_transformer_amd import multimodal_driver as D
    assert D.get_parser().parse_args([]).max_grad_norm == 0.0          # the reference does not clip
    assert D.get_parser().parse_args(["--max_grad_norm", "1.0"]).max_grad_norm == 1.0


def test_header_symbols_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    h = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(h, name), name
        assert name in _lib.PROTOTYPES, name
    L = _lib.lib()
    # the scratch is a function of n alone, one double per block, 2048 blocks at the most
    sizes = [L.mb_grad_clip_scratch_bytes(n) for n in (0, 1, 4099, 4100, 5000003, 111 * 10 ** 6, 337 * 10 ** 6, 2 ** 33)]
    assert sizes[0] == sizes[1] == sizes[2] == 8 and sizes[3] == 16 and sizes == sorted(sizes) and sizes[-1] == sizes[-2] == 2048 * 8, sizes


def _engine(kind):
    L = _lib.lib()
    h = C.c_void_p()
    if kind == "bert":
        cfg = _lib.BertEngineConfig(30522, 768, 2, 12, 3072, 512, 2, 1, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_bert_create(C.byref(cfg), C.byref(h)))
    else:
        cfg = _lib.XlnetEngineConfig(32000, 768, 2, 12, 3072, 1, 47, 74, 1, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, _lib.DT_BF16, 4, 50)
        _lib.check(L.mb_xlnet_create(C.byref(cfg), C.byref(h)))
    return L, (lambda name: getattr(L, "mb_%s_%s" % (kind, name))), h


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_engine_setting_on_the_host(kind):
    """off by default; the getter refuses while clipping is off or no update has run; the data-parallel step refuses while it is on,
    before it looks at anything else; the workspace does not grow"""
    L, fn, h = _engine(kind)
    ARG, MODE = 1004, 1002
    norm, coef = C.c_float(), C.c_float()
    ws = fn("workspace_bytes")(h)
    assert fn("grad_clip_stats")(h, C.byref(norm), C.byref(coef), None) == MODE
    dp = lambda: fn("train_step_dp")(h, None, None, None, None, None, None, 4, 50, 0, 1, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-6,
                                     0.01, 1, 1, 1.0, 1.0, 1, None, None)
    assert dp() == ARG
    assert fn("set_grad_clip")(h, 1.0) == 0
    assert fn("grad_clip_stats")(h, C.byref(norm), C.byref(coef), None) == MODE      # on, but no update has run
    assert dp() == MODE
    for off in (0.0, -2.0, float("inf"), float("nan")):
        assert fn("set_grad_clip")(h, 1.0) == 0 and dp() == MODE
        assert fn("set_grad_clip")(h, off) == 0 and dp() == ARG
    assert fn("workspace_bytes")(h) == ws
    assert fn("set_grad_clip")(None, 1.0) == ARG
    fn("destroy")(h)


def test_sharded_update_with_clipping_raises():
    """MB_DP_SHARD_OPT=1: a rank holds only its shard of the reduced gradient -- step() says so by name instead of clipping by a partial norm"""
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    opt = AdamW([p], lr=1e-3, max_grad_norm=1.0)

    class Dp(object):
        late_ranges = []
        shards = object()
        shard_in_engine = False
    opt._dp = Dp()
    with pytest.raises(_lib.MagbertError, match="MB_DP_SHARD_OPT"):
        opt.step()
    assert float(p.detach().abs().max()) == 0.0 and opt._t == 1
