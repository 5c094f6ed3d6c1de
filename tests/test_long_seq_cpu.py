"""CPU: the long-sequence surface of the library (tiled attention, engines with max_seq > 128) -- no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from bert_multimodal_transformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mb_attention_tiled_forward", "mb_attention_tiled_backward", "mb_attention_tiled_stats_bytes",
       "mb_attention_resident_forward", "mb_attention_resident_backward")


def _cfg(max_seq, max_position=512, max_batch=4):
    return _lib.BertEngineConfig(30522, 768, 2, 12, 3072, max_position, 2, 1, 47, 74, 0, 1e-12, 1e-5, 1.0, 0.1, 0.1, 0.5,
                                 _lib.DT_BF16, max_batch, max_seq)


def _create(cfg):
    h = C.c_void_p()
    rc = _lib.lib().mb_bert_create(C.byref(cfg), C.byref(h))
    return rc, h


def test_bert_engine_accepts_sequences_up_to_the_position_table():
    L = _lib.lib()
    sizes = {}
    for n in (128, 256, 512):
        rc, h = _create(_cfg(n))
        assert rc == 0, n
        sizes[n] = L.mb_bert_workspace_bytes(h)
        L.mb_bert_destroy(h)
    assert sizes[128] < sizes[256] < sizes[512]
    assert _create(_cfg(513))[0] == 1001                          # above 512
    assert _create(_cfg(300, max_position=256))[0] == 1001        # above the position table
    assert _create(_cfg(600, max_position=1024))[0] == 1001       # 512 is the kernels' limit whatever the table holds


def test_new_symbols_in_header_prototypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "magbert_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(L, name), name


def test_tiled_stats_bytes():
    L = _lib.lib()
    assert L.mb_attention_tiled_stats_bytes(2, 300, 12) == 3 * 2 * 12 * 300 * 4
    assert L.mb_attention_tiled_stats_bytes(0, 300, 12) == 0


def test_tiled_launchers_check_shapes_before_pointers():
    """dummy pointers: every call below must be refused before it could launch (skipped where a GPU could run a missed check)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    bogus = C.c_void_p(0x1000)
    key = _lib.make_dropkey(1, 1, 17, 0.1)
    fwd = lambda dt, B, S, nh, k: L.mb_attention_tiled_forward(dt, bogus, bogus, bogus, bogus, B, S, nh, k, None, None, None)
    bwd = lambda dt, B, S, nh, k: L.mb_attention_tiled_backward(dt, bogus, bogus, bogus, bogus, bogus, bogus, None, B, S, nh, k,
                                                                None, None)
    for f in (fwd, bwd):
        assert f(_lib.DT_BF16, 2, 513, 12, None) == 1001
        assert f(_lib.DT_BF16, 2, 0, 12, None) == 1001
        assert f(_lib.DT_BF16, 0, 256, 12, None) == 1001
        assert f(_lib.DT_BF16, 2, 256, 0, None) == 1001
        # dropout on and B * nh * L^2 >= 2^32: the uint32 mask index would wrap
        assert f(_lib.DT_BF16, 1366, 512, 12, C.byref(key)) == 1001
        assert f(_lib.DT_F32, 1366, 512, 12, C.byref(key)) == 1001
        assert f(7, 2, 256, 12, None) == 1003
    # the LDS-resident pair keeps its L <= 128 contract
    assert L.mb_attention_forward(_lib.DT_BF16, bogus, bogus, bogus, 2, 129, 12, None, None) == 1001
    assert L.mb_attention_backward(_lib.DT_BF16, bogus, bogus, bogus, bogus, 2, 129, 12, None, None) == 1001


def test_resident_launchers_check_shapes_before_pointers():
    """mb_attention_resident_forward / _backward (the LDS-resident kernels with head_scale, probs and dbias): the checks of the tiled
    pair, except that L > 128 is refused; dummy pointers, so skipped where a GPU could run a missed check"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    bogus = C.c_void_p(0x1000)
    key = _lib.make_dropkey(1, 1, 17, 0.1)
    fwd = lambda dt, B, S, nh, k: L.mb_attention_resident_forward(dt, bogus, bogus, bogus, B, S, nh, k, None, None, None)
    bwd = lambda dt, B, S, nh, k: L.mb_attention_resident_backward(dt, bogus, bogus, bogus, bogus, None, B, S, nh, k, None, None)
    for f in (fwd, bwd):
        assert f(_lib.DT_BF16, 2, 129, 12, None) == 1001
        assert f(_lib.DT_F32, 2, 512, 12, None) == 1001
        assert f(_lib.DT_BF16, 2, 0, 12, None) == 1001
        assert f(_lib.DT_BF16, 0, 128, 12, None) == 1001
        assert f(_lib.DT_BF16, 2, 128, 0, None) == 1001
        # dropout on and B * nh * L^2 >= 2^32: the uint32 mask index would wrap
        assert f(_lib.DT_BF16, 21846, 128, 12, C.byref(key)) == 1001
        assert f(_lib.DT_F32, 21846, 128, 12, C.byref(key)) == 1001
        assert f(7, 2, 128, 12, None) == 1003
    # null operands are refused after the shape (MB_ERR_ARG); the optional ones (head_scale, probs, dbias) may be null
    assert L.mb_attention_resident_forward(_lib.DT_BF16, None, bogus, bogus, 2, 128, 12, None, None, None, None) == 1004
    assert L.mb_attention_resident_forward(_lib.DT_BF16, bogus, None, bogus, 2, 128, 12, None, None, None, None) == 1004
    assert L.mb_attention_resident_forward(_lib.DT_BF16, bogus, bogus, None, 2, 128, 12, None, None, None, None) == 1004
    assert L.mb_attention_resident_backward(_lib.DT_BF16, bogus, bogus, None, bogus, None, 2, 128, 12, None, None, None) == 1004
    assert L.mb_attention_resident_backward(_lib.DT_BF16, bogus, bogus, bogus, None, None, 2, 128, 12, None, None, None) == 1004
    assert L.mb_attention_resident_forward(_lib.DT_BF16, None, bogus, bogus, 2, 129, 12, None, None, None, None) == 1001


def test_tiled_kernels_registers_and_lds(tmp_path):
    """code-object metadata of attention_tiled.o: the bf16 kernels spill nothing and keep at least two workgroups per CU; the
    forward is held by its LDS, not its registers (blocks per CU by registers >= by LDS)"""
    from bert_multimodal_transformer_amd import build as mb_build
    mb_build.build(verbose=False)
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    obj = shutil.copy(os.path.join(mb_build.LIBDIR, "obj", "attention_tiled.o"), tmp_path / "attention_tiled.o")
    subprocess.run([objdump, "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    notes = subprocess.run([readelf, "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s+-?\s*\.(name|vgpr_count|vgpr_spill_count|group_segment_fixed_size|wavefront_size):\s+(\S+)", line)
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "wavefront_size":
                kernels[cur["name"]] = (int(cur["vgpr_count"]), int(cur["group_segment_fixed_size"]), int(cur.get("vgpr_spill_count", 0)))
                cur = {}
    by_reg = lambda v: 512 // ((v + 7) // 8 * 8)           # waves per SIMD = 256-thread blocks per CU
    by_lds = lambda l: (160 * 1024) // l
    bf16 = {n: v for n, v in kernels.items() if "attn_tiled" in n and "DF16b" in n}
    assert len(bf16) == 3, sorted(kernels)
    for name, (vgpr, lds, spill) in bf16.items():
        assert spill == 0 and by_reg(vgpr) >= 2 and by_lds(lds) >= 2, (name, vgpr, lds, spill)
        if "fwd" in name:
            assert by_reg(vgpr) >= min(by_lds(lds), 8), (name, vgpr, lds)
