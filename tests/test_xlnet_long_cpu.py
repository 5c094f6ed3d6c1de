"""CPU: the long-sequence surface of MAG-XLNet (tiled relative attention, engines with max_seq > 128) -- no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from bert_multimodal_transformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mb_xlnet_attention_tiled_forward", "mb_xlnet_attention_tiled_backward", "mb_xlnet_attention_tiled_stats_bytes",
       "mb_xlnet_attention_tiled_scratch_bytes", "mb_xlnet_attention_forward", "mb_xlnet_attention_backward",
       "mb_xlnet_attention_probs_into")


def _cfg(max_seq, dtype=_lib.DT_BF16, max_batch=4):
    return _lib.XlnetEngineConfig(32000, 768, 12, 12, 3072, 1, 47, 74, 1, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5, dtype, max_batch, max_seq)


def _create(cfg):
    h = C.c_void_p()
    rc = _lib.lib().mb_xlnet_create(C.byref(cfg), C.byref(h))
    return rc, h


def _ws(max_seq, dtype):
    rc, h = _create(_cfg(max_seq, dtype))
    assert rc == 0, (max_seq, dtype)
    n = _lib.lib().mb_xlnet_workspace_bytes(h)
    _lib.lib().mb_xlnet_destroy(h)
    return n


def test_xlnet_engine_accepts_sequences_up_to_512(monkeypatch):
    monkeypatch.delenv("MB_DETERMINISTIC", raising=False)
    sizes = {n: _ws(n, _lib.DT_BF16) for n in (128, 256, 512)}
    assert sizes[128] < sizes[256] < sizes[512]
    assert _create(_cfg(513))[0] == 1001
    assert _create(_cfg(0))[0] == 1001
    # engines with max_seq <= 128 carve exactly what they carved before the tiled kernels existed (read from a build of the parent
    # commit with this configuration)
    assert sizes[128] == 255603968 and _ws(50, _lib.DT_BF16) == 126841088
    assert _ws(128, _lib.DT_F32) == 485260544 and _ws(50, _lib.DT_F32) == 236566784
    # above 128 the per-layer [B*nh][LP][LP] probabilities are gone: 12 layers of row statistics + two shared planes instead
    per_layer_probs = 4 * 12 * 512 * 512 * 2
    assert sizes[512] < 4 * sizes[128] + 2 * per_layer_probs


def test_new_symbols_in_header_prototypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(L, name), name


def test_tiled_stats_and_scratch_bytes():
    L = _lib.lib()
    assert L.mb_xlnet_attention_tiled_stats_bytes(2, 300, 12) == 2 * 2 * 12 * 300 * 4
    assert L.mb_xlnet_attention_tiled_stats_bytes(0, 300, 12) == 0
    assert L.mb_xlnet_attention_tiled_scratch_bytes(_lib.DT_BF16, 2, 300, 12) == 2 * 12 * 320 * 320 * 2      # rows and columns padded to 64
    assert L.mb_xlnet_attention_tiled_scratch_bytes(_lib.DT_F32, 2, 512, 12) == 2 * 12 * 512 * 512 * 4
    assert L.mb_xlnet_attention_tiled_scratch_bytes(7, 2, 512, 12) == 0


def test_launchers_check_shapes_before_pointers():
    """dummy pointers: every call below must be refused before it could launch (skipped where a GPU could run a missed check)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    g = C.c_void_p(0x1000)
    key = _lib.make_dropkey(1, 1, 17, 0.1)
    tf = lambda dt, B, S, nh, k: L.mb_xlnet_attention_tiled_forward(dt, g, g, g, g, g, g, g, g, g, g, B, S, nh, k, None, None, 0, None, None)
    tb = lambda dt, B, S, nh, k: L.mb_xlnet_attention_tiled_backward(dt, *([g] * 19), B, S, nh, k, None, None, None)
    of = lambda dt, B, S, nh, k: L.mb_xlnet_attention_forward(dt, *([g] * 11), B, S, nh, k, None, None, 0, None)
    ob = lambda dt, B, S, nh, k: L.mb_xlnet_attention_backward(dt, *([g] * 20), B, S, nh, k, None, None, None)
    for f in (tf, tb, of, ob):
        assert f(_lib.DT_BF16, 2, 513, 12, None) == 1001
        assert f(_lib.DT_BF16, 2, 0, 12, None) == 1001
        assert f(_lib.DT_BF16, 0, 256, 12, None) == 1001
        assert f(_lib.DT_BF16, 2, 256, 0, None) == 1001
        # dropout on and B * nh * L^2 >= 2^32: the uint32 mask index would wrap
        assert f(_lib.DT_BF16, 1366, 512, 12, C.byref(key)) == 1001
        assert f(_lib.DT_F32, 1366, 512, 12, C.byref(key)) == 1001
        assert f(7, 2, 256, 12, None) == 1003


def test_tiled_kernels_registers_and_lds(tmp_path):
    """code-object metadata of xlnet_attention_tiled.o: the four bf16 kernels spill nothing and keep at least two workgroups per CU,
    by registers and by LDS (the condition test_long_seq_cpu puts on the MAG-BERT kernels)"""
    from bert_multimodal_transformer_amd import build as mb_build
    mb_build.build(verbose=False)
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    obj = shutil.copy(os.path.join(mb_build.LIBDIR, "obj", "xlnet_attention_tiled.o"), tmp_path / "xlnet_attention_tiled.o")
    subprocess.run([objdump, "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    notes = subprocess.run([readelf, "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s+-?\s*\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size|wavefront_size):\s+(\S+)", line)
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "wavefront_size":
                kernels[cur["name"]] = (int(cur["vgpr_count"]), int(cur["group_segment_fixed_size"]), int(cur.get("vgpr_spill_count", 0)),
                                        int(cur.get("private_segment_fixed_size", 0)))
                cur = {}
    by_reg = lambda v: 512 // ((v + 7) // 8 * 8)           # waves per SIMD = 256-thread blocks per CU
    by_lds = lambda l: (160 * 1024) // l
    bf16 = {n: v for n, v in kernels.items() if "xl_tiled" in n and "DF16b" in n}
    assert len(bf16) == 4, sorted(kernels)
    for name, (vgpr, lds, spill, scratch) in bf16.items():
        assert spill == 0 and scratch == 0 and by_reg(vgpr) >= 2 and by_lds(lds) >= 2, (name, vgpr, lds, spill, scratch)
    # fp32 is the parity mode: its rings fit the 160 KB of one CU, one workgroup at a time
    fp32 = {n: v for n, v in kernels.items() if "xl_tiled" in n and "DF16b" not in n}
    assert len(fp32) == 4
    for name, (vgpr, lds, spill, scratch) in fp32.items():
        assert lds <= 160 * 1024 and scratch == 0, (name, lds, scratch)


def test_python_limits_without_a_gpu():
    from bert_multimodal_transformer_amd import bert
    assert bert._xl_seq_limit(None) == 128 and bert._xl_seq_limit(50) == 128 and bert._xl_seq_limit(300) == 300
    assert bert._xl_seq_limit(512) == 512 == bert.XLNET_MAX_SEQ
    for bad in (0, 513, 4096):
        with pytest.raises(ValueError):
            bert._xl_seq_limit(bad)
    import inspect
    from bert_multimodal_transformer_amd import xlnet
    for cls in (xlnet.MAG_XLNetModel, xlnet.MAG_XLNetForSequenceClassification):
        assert inspect.signature(cls.__init__).parameters["max_seq_length"].default is None


@pytest.mark.parametrize("B,L,seed", [(2, 256, 51), (2, 512, 53)])
def test_oracle_matches_the_reference_fixture(golden, B, L, seed):
    """the live oracle -- the yardstick of the GPU tests -- against what the reference's own xlnet.py returned
    (tests/golden/g10_xlnet_long.npz, written by scripts/make_golden_long.py, whose batch construction is imported)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from make_golden_long import long_batch
    from oracle import mag_xlnet_ref as X
    b = long_batch(B, L, seed)
    o = X.load_deterministic(X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(n_layer=12), X.MultimodalConfig(1.0, 0.5), 47, 74), "test").eval()
    t = lambda k: torch.from_numpy(b[k])
    with torch.no_grad():
        got = o(t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"))[0].numpy()
    ref = golden["g10_xlnet_long"]["logits/B%d_L%d_seed%d" % (B, L, seed)]
    assert ref.shape == got.shape and float(np.abs(got - ref).max()) <= 2e-5
    assert set(golden["g10_xlnet_long"].files) == {"logits/B2_L256_seed51", "logits/B2_L512_seed53"}
