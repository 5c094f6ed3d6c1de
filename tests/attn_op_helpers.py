"""Shared pieces of the operator-level attention tests (test_xlnet_long_gpu.py, test_long_seq_gpu.py, test_attention_resident_gpu.py,
test_attention_tiled_gpu.py): the fp64 restatement of XLNet's relative attention, one op-level case of either model with its device
tensors and calls, and the error table.  A plain module, not a conftest."""
import ctypes as C

import numpy as np
import torch

from bert_multimodal_transformer_amd import _lib, rng
from test_ops_gpu import DEV, _attn_ref, close, rnd, stream


def _xl_ref(qkv, kr, rwb, rrb, rsb, sege, seg, mask, perm, gstream, B, L, nh, pm):
    """fp64: the formulas of the header of csrc/xlnet_attention_tiled.hip.  pm [B, nh, L, L]: dropout multipliers x head_scale"""
    q, k, v = qkv.view(B, L, 3, nh, 64).permute(2, 0, 3, 1, 4)                     # [B, nh, L, 64]
    krh = kr.view(B, 2 * L, nh, 64).permute(0, 2, 1, 3)                             # [B, nh, 2L, 64]
    ac = (q + rwb[None, :, None, :]) @ k.transpose(-1, -2)
    bd_full = (q + rrb[None, :, None, :]) @ krh.transpose(-1, -2)                   # [B, nh, L, 2L]
    ar = torch.arange(L)
    idx = (L - ar[:, None] + ar[None, :]).expand(B, nh, L, L)
    bd = torch.gather(bd_full, -1, idx)
    ef2 = torch.einsum("bhid,shd->bhis", q + rsb[None, :, None, :], sege)            # [B, nh, L, 2]
    diff = (seg[:, :, None] != seg[:, None, :]).long()[:, None].expand(B, nh, L, L)
    ef = torch.gather(ef2, -1, diff)
    masked = (mask[:, None, :] == 0).expand(B, L, L).clone()
    if perm is not None:
        masked |= perm != 0
    if not gstream:
        masked &= ~torch.eye(L, dtype=torch.bool)[None]
    s = (ac + bd + ef) / 8.0 - 1e30 * masked[:, None].double()
    p = torch.softmax(s, -1)
    vec = (p * pm) @ v
    return vec.permute(0, 2, 1, 3).reshape(B * L, nh * 64), p


def xl_lp(L):
    """the padded length of the LDS-resident XLNet kernels (XL_DISPATCH in csrc/xlnet_attention.hip)"""
    return 32 if L <= 32 else (64 if L <= 64 else 128)


class _XlOp(object):
    """device tensors of one op-level case + the calls.  poison: the scratch (psave, gsave, pdsave) and the output tensors vec / dqkv /
    dkr hold NaN before the forward -- the kernels must write every element they own and never read a scratch row or column >= L.
    padded_sample: sample 1 has no real key at all (mask[1, :] = 0).  perm: True for a random one (30 %), or a given [B, L, L] tensor
    (non-zero = masked).  dev=None: no device tensors, for running reference() alone on a machine without a GPU."""

    def __init__(self, dt, tdt, B, L, nh, seed, p, perm=False, gstream=0, poison=False, padded_sample=False, dev=DEV):
        assert nh >= 4                                                       # hs[3] = 0 below
        self.dt, self.tdt, self.B, self.L, self.nh = dt, tdt, B, L, nh
        self.poison = poison
        H = nh * 64
        self.qkv = rnd((B * L, 3 * H), seed, tdt, 2.0)
        self.kr = rnd((B * 2 * L, H), seed + 1, tdt, 1.0)
        self.dvec = rnd((B * L, H), seed + 2, tdt)
        self.rwb, self.rrb, self.rsb = (rnd((nh, 64), seed + 3 + k, torch.float32, 0.5) for k in range(3))
        self.sege = rnd((2, nh, 64), seed + 6, torch.float32, 0.5)
        self.mask = torch.ones(B, L, dtype=torch.long)
        self.mask[1, :L - 5] = 0                                             # row 1: left-padded down to 5 real keys
        if padded_sample:
            self.mask[1, :] = 0
        self.seg = torch.zeros(B, L, dtype=torch.long)
        self.seg[:, L - 1] = 2
        self.seg[0, L // 3: L // 2] = 1
        self.seg[1, :L - 5] = 3
        self.hs = torch.linspace(0.5, 1.5, nh, dtype=torch.float32)
        self.hs[3] = 0.0
        self.perm = None
        if isinstance(perm, torch.Tensor):
            assert tuple(perm.shape) == (B, L, L)
            self.perm = perm.to(torch.uint8).clone()
        elif perm:
            self.perm = (torch.from_numpy(np.random.RandomState(seed).rand(B, L, L) < 0.3)).to(torch.uint8)
        self.gstream = gstream
        if gstream:                                                          # a query row that may attend to nothing at all
            self.perm = torch.zeros(B, L, L, dtype=torch.uint8) if self.perm is None else self.perm
            self.perm[0, L // 2, :] = 1
            self.perm[1, L - 2, :] = 1
        self.key, self.pmask = None, torch.ones(B, nh, L, L, dtype=torch.float64)
        if p > 0:
            self.key = _lib.make_dropkey(7, 5, 16, p)
            self.pmask = torch.from_numpy(rng.keep_mult(B * nh * L * L, rng.make_key(7, 5, 16, p))).view(B, nh, L, L).double()
        d = lambda t, ty=None: t.to(dev, ty) if ty is not None else t.to(dev)
        self.d = None if dev is None else dict(qkv=d(self.qkv, tdt), kr=d(self.kr, tdt), dvec=d(self.dvec, tdt), rwb=d(self.rwb), rrb=d(self.rrb), rsb=d(self.rsb),
                      sege=d(self.sege), mask=d(self.mask), seg=d(self.seg), hs=d(self.hs), perm=d(self.perm) if self.perm is not None else None)
        self.ref_probs = None          # [B, nh, L, L] fp64, the softmax before dropout: set by reference()
        self.psave = None              # [B * nh, LP, LP], what the last resident forward saved: set by run(tiled=False)

    def reference(self, backward=True):
        leaves = [t.double().requires_grad_(backward) for t in (self.qkv, self.kr, self.rwb, self.rrb, self.rsb, self.sege)]
        pm = self.pmask * self.hs.double()[None, :, None, None]
        vec, probs = _xl_ref(*leaves, self.seg, self.mask, self.perm, self.gstream, self.B, self.L, self.nh, pm)
        self.ref_probs = probs.detach()
        grads = None
        if backward:
            vec.backward(self.dvec.double())
            grads = [t.grad for t in leaves]
        return vec.detach(), grads

    def _common(self):
        d = self.d
        return [_lib.ptr(d[k]) for k in ("qkv", "kr", "rwb", "rrb", "rsb", "sege", "seg", "mask")]

    def run(self, tiled, backward=True, param_grads=True):
        """-> vec, dqkv, dkr, (d_rwb, d_rrb, d_rsb, d_seg)"""
        L_, d = _lib.lib(), self.d
        dt, tdt, B, L, nh = self.dt, self.tdt, self.B, self.L, self.nh
        H = nh * 64
        kp = C.byref(self.key) if self.key is not None else None
        fill = float("nan") if self.poison else 0.0
        buf = lambda *shape: torch.full(shape, fill, dtype=tdt, device=DEV)
        vec = buf(B * L, H)
        stats = torch.zeros(L_.mb_xlnet_attention_tiled_stats_bytes(B, L, nh) // 4, dtype=torch.float32, device=DEV)
        es = 2 if tdt == torch.bfloat16 else 4
        nsc = L_.mb_xlnet_attention_tiled_scratch_bytes(dt, B, L, nh) // es
        LP = xl_lp(L)
        psave = None if tiled else buf(B * nh * LP * LP)
        gsave = buf(max(nsc, B * nh * LP * LP))
        pdsave = buf(nsc)
        dqkv, dkr = (buf(B * L, 3 * H), buf(B * 2 * L, H)) if backward else (None, None)
        if tiled:
            _lib.check(L_.mb_xlnet_attention_tiled_forward(dt, *self._common(), _lib.ptr(vec), _lib.ptr(stats), B, L, nh, kp, _lib.ptr(d["hs"]),
                                                           _lib.ptr(d["perm"]), self.gstream, None, stream()))
        else:
            _lib.check(L_.mb_xlnet_attention_forward(dt, *self._common(), _lib.ptr(vec), _lib.ptr(psave), _lib.ptr(stats), B, L, nh, kp,
                                                     _lib.ptr(d["hs"]), _lib.ptr(d["perm"]), self.gstream, stream()))
            self.psave = psave.view(B * nh, LP, LP)
        if not backward:
            torch.cuda.synchronize()
            return vec, None, None, None
        pg = [torch.zeros(nh, 64, device=DEV), torch.zeros(nh, 64, device=DEV), torch.zeros(nh, 64, device=DEV), torch.zeros(2, nh, 64, device=DEV)]
        tail = [_lib.ptr(dqkv), _lib.ptr(dkr)] + [_lib.ptr(t) for t in pg] + [B, L, nh, kp, _lib.ptr(d["hs"]), _lib.ptr(d["perm"]), stream()]
        if tiled:
            _lib.check(L_.mb_xlnet_attention_tiled_backward(dt, *self._common(), _lib.ptr(vec), _lib.ptr(d["dvec"]), _lib.ptr(stats),
                                                            _lib.ptr(gsave), _lib.ptr(pdsave), *tail))
        else:
            _lib.check(L_.mb_xlnet_attention_backward(dt, *self._common(), _lib.ptr(psave), _lib.ptr(vec), _lib.ptr(d["dvec"]), _lib.ptr(stats),
                                                      _lib.ptr(gsave), _lib.ptr(pdsave), *tail))
        torch.cuda.synchronize()
        return vec, dqkv, dkr, pg


NAMES = ("dqkv", "dkr", "d_rwb", "d_rrb", "d_rsb", "d_seg")


def _errors(case, got, ref_vec, ref_grads):
    """max |err| / max |ref| of every quantity"""
    vec, dqkv, dkr, pg = got
    out = {"vec": (vec.float().cpu(), ref_vec)}
    if dqkv is not None:
        for name, g, r in zip(NAMES, [dqkv, dkr] + list(pg), ref_grads):
            out[name] = (g.float().cpu().view(r.shape), r)
    return {k: (float((g.double() - r.double()).abs().max()), float(r.abs().max())) for k, (g, r) in out.items()}


# ------------------------------------------------------------------------------------------------------------ MAG-BERT
class _BertOp(object):
    """one op-level case of the BERT attention core: inputs, the fp64 reference (ctx, dqkv, the probabilities after dropout and head
    mask) and the device tensors.  mask [B, S]; family: the kernels the error table names; dev=None: the reference alone"""

    def __init__(self, dt, tdt, S, nh, p, mask, hs=None, family="resident", dev=DEV):
        B = mask.shape[0]
        self.dt, self.tdt, self.B, self.S, self.nh, self.family = dt, tdt, B, S, nh, family
        H = nh * 64
        self.qkv = rnd((B * S, 3 * H), 1, tdt, 2.0).requires_grad_(True)
        self.dctx = rnd((B * S, H), 2, tdt)
        self.key, pm = None, torch.ones(B, nh, S, S, dtype=torch.float64)
        if p > 0:
            self.key = _lib.make_dropkey(7, 5, 16, p)
            pm = torch.from_numpy(rng.keep_mult(B * nh * S * S, rng.make_key(7, 5, 16, p))).view(B, nh, S, S).double()
        if hs is not None:
            pm = pm * hs.double()[None, :, None, None]
        self.ctx = _attn_ref(self.qkv.double(), mask, B, S, nh, pm)
        self.ctx.backward(self.dctx.double())
        q, k, _ = self.qkv.detach().double().view(B, S, 3, nh, 64).permute(2, 0, 3, 1, 4)
        self.soft = torch.softmax(q @ k.transpose(-1, -2) / 8.0 + (1.0 - mask[:, None, None, :].double()) * -10000.0, -1)
        self.probs = self.soft * pm
        if dev is not None:
            self.qd, self.md, self.dcd = self.qkv.detach().to(dev, tdt), mask.to(dev), self.dctx.to(dev, tdt)
            self.hsd = hs.to(dev) if hs is not None else None
        self.kp = C.byref(self.key) if self.key is not None else None

    def references(self):
        return dict(ctx=self.ctx.detach(), dqkv=self.qkv.grad, probs=self.probs, dbias=self.qkv.grad.double().sum(0))

    def errors(self, what, **got):
        ref = self.references()
        for k, g in got.items():
            print("%s bert attention %s %s S=%d nh=%d %s: max|err| %.3e (max|ref| %.3e)"
                  % (self.family, what, self.tdt, self.S, self.nh, k, float((g.float().cpu().double() - ref[k].double()).abs().max()),
                     float(ref[k].abs().max())))
        for k, g in got.items():
            close(g.float(), ref[k].float(), self.dt, what + " " + k, 2.0 if k in ("ctx", "probs") else 3.0)


def _tiled(dt, tdt, qd, md, dctx_d, B, S, nh, key, hs=None, probs=False, dbias=False, poison=False):
    """mb_attention_tiled_forward / _backward -> ctx, dqkv, probs, dbias.  poison: ctx, probs, dqkv and the three stats planes hold NaN
    before the forward (dbias is accumulated into, so it starts from zero)"""
    L = _lib.lib()
    H = nh * 64
    fill = float("nan") if poison else 0.0
    stats = torch.full((L.mb_attention_tiled_stats_bytes(B, S, nh) // 4,), fill, dtype=torch.float32, device=DEV)
    out = torch.full((B * S, H), fill, dtype=tdt, device=DEV)
    pr = torch.full((B, nh, S, S), fill, dtype=torch.float32, device=DEV) if probs else None
    kp = C.byref(key) if key is not None else None
    _lib.check(L.mb_attention_tiled_forward(dt, _lib.ptr(qd), _lib.ptr(md), _lib.ptr(out), _lib.ptr(stats), B, S, nh, kp,
                                            _lib.ptr(hs), _lib.ptr(pr), stream()))
    dq = torch.full((B * S, 3 * H), fill, dtype=tdt, device=DEV)
    db = torch.zeros(3 * H, dtype=torch.float32, device=DEV) if dbias else None
    _lib.check(L.mb_attention_tiled_backward(dt, _lib.ptr(qd), _lib.ptr(md), _lib.ptr(out), _lib.ptr(dctx_d), _lib.ptr(stats),
                                             _lib.ptr(dq), _lib.ptr(db), B, S, nh, kp, _lib.ptr(hs), stream()))
    torch.cuda.synchronize()
    return out, dq, pr, db
