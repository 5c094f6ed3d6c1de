"""GPU: the moment-skip path of the end-of-step sweep (csrc/adamw_dev.h adam_span: adam_load_p / adam_decay_store; csrc/kernels.h WordSkip,
MB_STAMP_SEEN) through the test hook mb_debug_adamw_sweep, and the scan behind the seen marks (csrc/rowops.hip word_moments_scan_kernel)
through mb_debug_word_moments_scan.

A flat buffer is laid out as  guard | 20 quads of another tensor | the word range | a position-table-like piece | guard.  The word range
begins 84 quads into the buffer -- no multiple of 64, so waves straddle rows whose states differ -- and the next piece follows it
directly.  A row is live (stamped with this update's number), seen (an older number with the seen mark, non-zero moments, g = +0.0f) or
unseen (no mark, m = v = g = +0.0f); the pattern is rotated so that the first and the last row take each state in turn.

Reference: the SAME launch with state[2] = 0, i.e. the sweep that reads and writes every moment: p, m, v, g and the bf16 shadow must be
bit-equal (torch.equal), guards included.  On top of that p is compared with oracle/optim_ref.py's AdamW on the CPU within the bound of
test_ops_gpu.test_adamw_kernel_matches_hf_formula (2e-6 max|ref|)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import _lib

DEV = "cuda:0"
SEEN = 0x80000000
NO = 7                      # this update's number
GUARD = 256                 # floats in front of and behind everything
PRE = 80                    # floats of the tensor in front of the word range (20 quads)
LR, B1, B2, EPS, WD, T, GSCALE = 1e-3, 0.9, 0.999, 1e-6, 0.01, 3, 0.5
CANARY = 1536.0             # (a bf16 too)
DECAY = float(np.float32(LR) * np.float32(WD))          # the float the device forms: lr * weight_decay in fp32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _layout(rows, row_len):
    wb = GUARD + PRE
    we = wb + rows * row_len
    pos = 520                # floats of the piece behind the table: two full blocks of quads and a ragged end
    return wb, we, we + pos, we + pos + GUARD


def _state_of(r, rot):
    return ("live", "seen", "unseen")[(r + rot) % 3]


def _buffers(rows, row_len, rot, seed):
    wb, we, end, n = _layout(rows, row_len)
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.1
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-3
    stamp = np.zeros(rows + 16, np.uint32)          # 8 guard words on either side (read-only for the sweep)
    stamp[:8] = NO; stamp[-8:] = NO
    for r in range(rows):
        a, b = wb + r * row_len, wb + (r + 1) * row_len
        st = _state_of(r, rot)
        if st == "live":
            stamp[8 + r] = NO | (SEEN if r % 2 else 0)          # (a live row is live with or without the mark)
        elif st == "seen":
            stamp[8 + r] = (NO - 1 - r % 3) | SEEN
            gr[a:b] = 0.0
        else:
            stamp[8 + r] = (NO - 1 - r % 3) if r % 2 else 0
            gr[a:b] = 0.0; m[a:b] = 0.0; v[a:b] = 0.0
    for t in (p, gr, m, v):
        t[:GUARD] = CANARY; t[end:] = CANARY
    return p, gr, m, v, stamp


def _cls_table():
    ss = LR * math.sqrt(1.0 - B2 ** T) / (1.0 - B1 ** T)
    rows = [[LR, B1, B2, EPS, WD, ss, GSCALE], [LR, B1, B2, EPS, 0.0, ss, GSCALE]]
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


def _launch(rows, row_len, rot, word_slot, shadow_mode, lazy, seed=3):
    L = _lib.lib()
    wb, we, end, n = _layout(rows, row_len)
    p, gr, m, v, stamp = _buffers(rows, row_len, rot, seed)
    dev = [t.clone().to(DEV) for t in (p, gr, m, v)]
    sh = torch.full((n,), CANARY, dtype=torch.bfloat16, device=DEV)
    shb, she = {"all": (GUARD, end), "half": (GUARD, wb + (rows // 2) * row_len + 8), "none": (0, 0)}[shadow_mode]
    st = torch.from_numpy(stamp.view(np.int32)).to(DEV)
    state = torch.from_numpy(np.array([NO, 1, 1 if lazy else 0, 0], np.uint32).view(np.int32)).to(DEV)
    cls = _cls_table()
    u32 = lambda xs: (_lib.C.c_uint32 * len(xs))(*xs)
    begin4 = u32([GUARD // 4, we // 4]); len4 = u32([(we - GUARD) // 4, (end - we) // 4])
    slot = (_lib.C.c_uint8 * 2)(word_slot, 1 - word_slot)
    rc = L.mb_debug_adamw_sweep(_lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(sh), 2, begin4, len4, slot,
                                shb, she, 0, 0, _lib.ptr(cls), st.data_ptr() + 32, _lib.ptr(state), wb, we, row_len, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert torch.equal(st.cpu(), torch.from_numpy(stamp.view(np.int32))), "the sweep wrote into the stamp table"
    return dict(p=dev[0].cpu(), g=dev[1].cpu(), m=dev[2].cpu(), v=dev[3].cpu(), sh=sh.cpu(), host=(p, gr, m, v), span=(wb, we, end, n),
                shadow=(shb, she))


def _oracle(host, span, word_slot):
    from oracle import optim_ref as O
    p, gr, m, v = host
    wb, we, end, n = span
    parts = ((GUARD, we, word_slot), (we, end, 1 - word_slot))
    out = p.clone()
    for a, b, s in parts:
        q = torch.nn.Parameter(p[a:b].clone())
        opt = O.AdamW([{"params": [q], "weight_decay": WD if s == 0 else 0.0}], lr=LR, betas=(B1, B2), eps=EPS)
        opt.state[q] = {"step": T - 1, "exp_avg": m[a:b].clone(), "exp_avg_sq": v[a:b].clone()}
        q.grad = gr[a:b] * GSCALE
        opt.step()
        out[a:b] = q.detach()
    return out


@pytest.mark.parametrize("row_len", [256, 768])
@pytest.mark.parametrize("rows", [5, 37])
def test_moment_skip_path_keeps_the_bits(rows, row_len):
    """every rotation of the three row states x decay / no-decay slot x shadow over all, half and none of the table"""
    checked = 0
    for rot in range(3):
        for word_slot in (0, 1):
            for shadow_mode in ("all", "half", "none"):
                if shadow_mode != "all" and rot != word_slot:          # (the partial shadows once per slot: the launch count stays small)
                    continue
                ref = _launch(rows, row_len, rot, word_slot, shadow_mode, lazy=False)
                new = _launch(rows, row_len, rot, word_slot, shadow_mode, lazy=True)
                what = (rows, row_len, rot, word_slot, shadow_mode)
                for k in ("p", "m", "v", "g", "sh"):
                    assert torch.equal(new[k], ref[k]), (what, k)
                wb, we, end, n = new["span"]
                for k in ("p", "m", "v", "g"):          # canaries
                    assert bool((new[k][:GUARD] == CANARY).all()) and bool((new[k][end:] == CANARY).all()), (what, k)
                shb, she = new["shadow"]
                sh = new["sh"].float()
                assert bool((sh[:shb] == CANARY).all()) and bool((sh[she:] == CANARY).all()) if she else bool((sh == CANARY).all()), what
                if she:
                    assert torch.equal(new["sh"][shb:she], new["p"][shb:she].to(torch.bfloat16)), what
                # gradients: consumed where they were read (live rows, the other pieces), +0.0f everywhere else already
                assert float(new["g"][GUARD:end].abs().max()) == 0.0, what
                oracle = _oracle(new["host"], new["span"], word_slot)
                err = float((new["p"][GUARD:end] - oracle[GUARD:end]).abs().max())
                assert err <= 2e-6 * float(oracle[GUARD:end].abs().max()), (what, err)
                # the rows that take the short path exist, and moved by the decay alone
                p0 = new["host"][0]
                for r in range(rows):
                    if _state_of(r, rot) == "unseen":
                        a, b = wb + r * row_len, wb + (r + 1) * row_len
                        want = p0[a:b] - DECAY * p0[a:b] if word_slot == 0 else p0[a:b]
                        assert torch.equal(new["p"][a:b], want), (what, r)
                        assert float(new["m"][a:b].abs().max()) == 0.0 and float(new["v"][a:b].abs().max()) == 0.0, (what, r)
                        checked += 1
    assert checked > 0


def test_short_path_does_not_touch_moments():
    """the short path really runs: finite sentinels in m, v and g of an unseen row survive the launch that has the verdict, and are
    consumed by the one that has not"""
    rows, row_len, rot = 5, 256, 1          # rows 2 is unseen ((2 + 1) % 3 == 0 is live; (1 + 1) % 3 == 2)
    r = next(r for r in range(rows) if _state_of(r, rot) == "unseen")
    L = _lib.lib()
    wb, we, end, n = _layout(rows, row_len)
    out = {}
    for lazy in (True, False):
        p, gr, m, v, stamp = _buffers(rows, row_len, rot, 5)
        a, b = wb + r * row_len, wb + (r + 1) * row_len
        m[a:b] = 123.0; v[a:b] = 123.0; gr[a:b] = 123.0
        dev = [t.clone().to(DEV) for t in (p, gr, m, v)]
        st = torch.from_numpy(stamp.view(np.int32)).to(DEV)
        state = torch.from_numpy(np.array([NO, 1, 1 if lazy else 0, 0], np.uint32).view(np.int32)).to(DEV)
        cls = _cls_table()
        u32 = lambda xs: (_lib.C.c_uint32 * len(xs))(*xs)
        rc = L.mb_debug_adamw_sweep(_lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), None, 1, u32([GUARD // 4]),
                                    u32([(end - GUARD) // 4]), (_lib.C.c_uint8 * 1)(0), 0, 0, 0, 0, _lib.ptr(cls), st.data_ptr() + 32,
                                    _lib.ptr(state), wb, we, row_len, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        out[lazy] = [t.cpu()[a:b] for t in dev] + [p[a:b]]
    pl, gl, ml, vl, p0 = out[True]
    assert bool((ml == 123.0).all()) and bool((vl == 123.0).all()) and bool((gl == 123.0).all())
    assert torch.equal(pl, p0 - DECAY * p0)
    pf, gf, mf, vf, _ = out[False]
    assert bool((mf == float(np.float32(B1) * np.float32(123.0))).all()) and bool((gf == 123.0).all()) and not torch.equal(pf, pl)


@pytest.mark.parametrize("row_len", [256, 768])
def test_scan_marks_exactly_the_rows_with_a_set_bit(row_len):
    """37 rows (ten blocks of four, the last one ragged): a row is marked when any bit of its m or v is set -- one element at the row's
    start, at its end, -0.0f, a denormal --, unmarked when both are all +0.0f whatever its mark was, and left alone when it carries keep_no"""
    L = _lib.lib()
    rows, begin, keep = 37, 84 * 4, 9
    n = begin + rows * row_len + 64
    m = torch.zeros(n); v = torch.zeros(n)
    m[:begin] = 1.0; v[:begin] = 1.0; m[begin + rows * row_len:] = 1.0; v[begin + rows * row_len:] = 1.0      # neighbours: never read
    want = np.zeros(rows, bool)
    marks = {1: ("m", 0, 1.0), 2: ("v", row_len - 1, 1.0), 5: ("m", row_len - 1, -0.0), 6: ("v", 0, 1e-45), 36: ("v", row_len // 2 + 1, 3.0),
             35: ("m", 65, 2.0)}
    for r, (which, at, val) in marks.items():
        (m if which == "m" else v)[begin + r * row_len + at] = val
        want[r] = True
    stamp = np.zeros(rows + 16, np.uint32)
    stamp[:8] = 0x12345678; stamp[-8:] = 0x12345678
    for r in range(rows):
        stamp[8 + r] = (r % 5) | (SEEN if r % 2 else 0)          # numbers 0 .. 4 (never keep_no), marks set on the odd rows
    stamp[8 + 10] = keep                                          # all-zero moments, no mark: stays unmarked
    stamp[8 + 11] = keep | SEEN                                   # all-zero moments, marked: stays marked
    stamp[8 + 1] = keep                                           # non-zero moments, no mark, keep_no: stays unmarked too
    exp = stamp.copy()
    for r in range(rows):
        if (stamp[8 + r] & ~np.uint32(SEEN)) != keep:
            exp[8 + r] = (stamp[8 + r] & ~np.uint32(SEEN)) | (np.uint32(SEEN) if want[r] else np.uint32(0))
    st = torch.from_numpy(stamp.view(np.int32)).to(DEV)
    md, vd = m.to(DEV), v.to(DEV)
    rc = L.mb_debug_word_moments_scan(_lib.ptr(md), _lib.ptr(vd), st.data_ptr() + 32, begin, rows, row_len, keep, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = st.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, exp), np.nonzero(got != exp)
    assert torch.equal(md.cpu(), m) and torch.equal(vd.cpu(), v)
