"""GPU: global gradient-norm clipping -- the norm operator (mb_grad_clip_coef) and clipping inside the single-call training step.

Adam's update m / (sqrt(v) + eps) is almost invariant to the gradient's scale, so a wrong coefficient hardly shows in the parameters:
the model tests assert the moments.  Yardsticks: numpy fp64 for the operator; for the step, train_step(..., graph=False) =
training_step + optimizer.step() with the same max_grad_norm (bit for bit in deterministic mode), the fp64 norm over the named
parameters' `.grad` tensors (not the flat buffer: dirty alignment padding would show), and the CPU oracle with
torch.nn.utils.clip_grad_norm_.

The model tests share one setup: three layers, the small shapes (5, 40) and (3, 24), the labels of odd updates multiplied by 8 so that
the gradient norms differ, max_norm = the geometric mean of the smallest and largest norm of the same trajectory run unclipped."""
import contextlib
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bert_multimodal_transformer_amd import (AdamW, BertConfig, MAG_BertForSequenceClassification, MAG_XLNetForSequenceClassification,
                                             MultimodalConfig, XLNetConfig, get_linear_schedule_with_warmup, layerwise_lr_groups, _lib)
from bert_multimodal_transformer_amd.multimodal_driver import optimizer_grouped_parameters
from oracle import mag_bert_ref as R
from oracle import mag_xlnet_ref as X
from oracle import optim_ref as O
from oracle import weights

DEV = "cuda:0"
LR, DECAY, HEAD = 1e-3, 0.5, 5e-3
SMALL = ((5, 40), (5, 40), (3, 24), (5, 40))


# ------------------------------------------------------------------------------------------------ the operator
def clip_op(g, max_norm, grad_scale):
    """{norm, coef} of mb_grad_clip_coef over the device tensor g; the scratch is NaN before the call"""
    L = _lib.lib()
    n = g.numel()
    nbytes = L.mb_grad_clip_scratch_bytes(n)
    assert 8 <= nbytes <= 2048 * 8
    scratch = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(L.mb_grad_clip_coef(g.data_ptr(), n, float(max_norm), float(grad_scale), scratch.data_ptr(), out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


def on_device(host, offset):
    """host fp32 array on the device, its base pointer `offset` floats past a 16-byte boundary"""
    buf = torch.empty(host.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    g = buf[offset: offset + host.size]
    g.copy_(torch.from_numpy(host))
    assert g.data_ptr() % 16 == 4 * offset
    return g


def f32(x):
    return float(np.float32(x))


def check_op(host, big_norm=True):
    """norm to 1e-6 of numpy fp64 (fp32 rounding of the result: 6e-8; the double sum is far below that), coef within one fp32 ulp of
    min(1, max_norm / (norm64 + 1e-6)), for max_norm above and below the norm, grad_scale 1 and 0.5, base pointer aligned and one float
    off, and the same bits on a second run.  big_norm: the norm is far above the formula's 1e-6, so max_norm >= 2 * norm gives exactly 1."""
    sum64 = float(np.sum(host.astype(np.float64) ** 2))
    for offset in (0, 1):
        g = on_device(host, offset)
        for gs in (1.0, 0.5):
            norm64 = gs * math.sqrt(sum64)
            for mx in (f32(2.5 * norm64), f32(0.3 * norm64)):
                got = clip_op(g, mx, gs)
                again = clip_op(g, mx, gs)
                assert got.tobytes() == again.tobytes(), (host.size, offset, got, again)
                want = min(1.0, mx / (norm64 + 1e-6))
                print("n=%d offset=%d gs=%g max_norm=%.6g: norm %.9g (fp64 %.9g) coef %.9g (fp64 %.9g)" % (host.size, offset, gs, mx, got[0], norm64, got[1], want))
                assert abs(float(got[0]) - norm64) <= 1e-6 * norm64, (host.size, offset, gs, got, norm64)
                assert abs(float(got[1]) - float(np.float32(want))) <= float(np.spacing(np.float32(want))), (host.size, offset, gs, mx, got, want)
                if big_norm and mx >= 2.0 * norm64:
                    assert float(got[1]) == 1.0
                if mx < 0.5 * norm64:
                    assert float(got[1]) < 1.0


@pytest.mark.parametrize("n", [1, 3, 1023, 4 * 1024 + 5, 2 ** 20 + 7, 5000003])
def test_norm_operator_sizes_and_alignment(n):
    host = np.random.RandomState(n % 9973).standard_normal(n).astype(np.float32)
    check_op(host)


@pytest.mark.parametrize("n", [4 * 1024 + 5, 2 ** 20 + 7])
def test_norm_operator_squares_outside_fp32(n):
    """a few 1e20 values (their squares overflow fp32) among normal ones, and a buffer of 1e-30 values (their squares underflow fp32):
    every element is widened to double before it is squared.  The tiny buffer's norm is far below the 1e-6 of the formula, so its
    coefficient is below 1 for any max_norm near the norm: the formula is the yardstick there."""
    rs = np.random.RandomState(7)
    host = rs.standard_normal(n).astype(np.float32)
    host[rs.choice(n, 5, replace=False)] = np.float32(1e20) * np.array([1, -1, 2, -0.5, 1.5], dtype=np.float32)
    check_op(host)
    tiny = (np.float32(1e-30) * (1.0 + rs.rand(n))).astype(np.float32)
    assert float(np.sum(tiny.astype(np.float32) ** 2, dtype=np.float32)) == 0.0          # (what an fp32 square would have summed)
    check_op(tiny, big_norm=False)


def test_norm_operator_nan_element_gives_nan_norm():
    host = np.random.RandomState(3).standard_normal(2 ** 20 + 7).astype(np.float32)
    host[777777] = np.nan
    got = clip_op(on_device(host, 1), 1.0, 1.0)
    assert np.isnan(got[0]) and np.isnan(got[1]), got
    host[777777] = np.inf
    got = clip_op(on_device(host, 0), 1.0, 1.0)
    assert np.isinf(got[0]) and got[1] == 0.0, got


# ------------------------------------------------------------------------------------------------ the shared model setup
@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(kind, layers, cdt, dropout=True):
    p, pm = (0.1, 0.5) if dropout else (0.0, 0.0)
    if kind == "bert":
        cfg = BertConfig(num_hidden_layers=layers, num_labels=1, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
        m = MAG_BertForSequenceClassification(cfg, MultimodalConfig(1.0, pm), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    else:
        cfg = XLNetConfig(n_layer=layers, num_labels=1, dropout=p, summary_last_dropout=p)
        m = MAG_XLNetForSequenceClassification(cfg, MultimodalConfig(1.0, pm), visual_dim=47, acoustic_dim=74, compute_dtype=cdt)
    m.load_state_dict({n: torch.from_numpy(weights.make_param(n, tuple(q.shape), "test")) for n, q in m.named_parameters()})
    return m


def batch(kind, B, L, seed, dev=DEV, label_mult=1.0):
    b = (weights.synthetic_bert_batch if kind == "bert" else weights.synthetic_xlnet_batch)(B, L, 47, 74, seed=seed)
    t = lambda k: torch.from_numpy(b[k]).to(dev)
    return t("input_ids"), t("visual"), t("acoustic"), t("input_mask"), t("segment_ids"), t("label_ids") * label_mult


def tensor_norm64(m):
    """fp64 norm over the named parameters' `.grad` tensors"""
    m.materialize_grads()
    tot = torch.zeros((), dtype=torch.float64, device=DEV)
    for _, p in m.named_parameters():
        if p.grad is not None:
            tot += p.grad.detach().double().pow(2).sum()
    return float(tot.sqrt())


def trajectory(kind, cdt, mode, max_norm=None, shapes=SMALL, nsteps=4, accum=1, layers=3, groups="driver", change=None, by_hand=False):
    """nsteps optimizer updates (dropout on, schedule moving, the labels of odd updates times 8) through model.train_step.  mode: False =
    training_step + optimizer.step(), True = step prologue + replayed graph, 2 = prologue + the same kernels launched one by one.
    by_hand (mode False only): the same three calls made here, with the fp64 norms of the flat gradient range and of the `.grad` tensors
    read in front of every update.  change = (update, value): max_grad_norm is set to `value` by hand before that update.
    Always in deterministic mode.  Returns tensors and records only -- no model -- so that runs can be cached."""
    with env(MB_DETERMINISTIC=1):
        torch.manual_seed(77)
        m = build(kind, layers, cdt).train()
        gs = layerwise_lr_groups(m.named_parameters(), layers, LR, layer_decay=DECAY, head_lr=HEAD) if groups == "classed" else optimizer_grouped_parameters(m)
        opt = AdamW(gs, lr=LR, max_grad_norm=max_norm)
        assert opt.max_grad_norm == max_norm
        sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
        core = m._core
        clip, flat64, tensor64, upd = [], [], [], []
        with m.stream_scope():
            for s in range(nsteps * accum):
                B, L = shapes[s % len(shapes)]
                u = s // accum
                data = batch(kind, B, L, 90 + s, label_mult=8.0 if u % 2 == 1 else 1.0)
                update = (s + 1) % accum == 0
                if change is not None and update and u == change[0]:
                    opt.max_grad_norm = change[1]
                if mode == 2:
                    o = opt.flat_step_args(core) if update else None
                    if update:
                        opt._t += 1
                        o["t"] = opt._t
                    core.train_step(*data, o, loss_scale=1.0 / accum, mode=2)
                    if update and o.get("max_grad_norm"):
                        opt._clip_last = core
                elif mode is False and by_hand:
                    m.training_step(*data, loss_scale=1.0 / accum)
                    if update:
                        flat64.append(float(m.flat_grads[: core.n_update_end].double().norm()))
                        tensor64.append(tensor_norm64(m))
                        opt.step()
                        opt.zero_grad()
                else:
                    m.train_step(*data, optimizer=opt if update else None, loss_scale=1.0 / accum, graph=mode)
                if update:
                    sch.step()
                    if opt.max_grad_norm:
                        clip.append(opt.last_grad_clip)
                        assert opt.last_grad_norm == clip[-1][0]
                    if mode is not False:
                        upd.append(core.update_stats())
        stats = core.graph_stats()
        m.eval()
        data = batch(kind, 4, 40, 99)
        with torch.no_grad():
            logits = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].clone()
        torch.cuda.synchronize()
        return dict(p=m.flat_params.clone(), m=core._adam_m.clone(), v=core._adam_v.clone(), gmax=float(m.flat_grads.abs().max()), logits=logits,
                    shadow=core.shadow.clone(), stats=stats, update=upd, clip=clip, flat64=flat64, tensor64=tensor64, n=core.n_update_end)


@functools.lru_cache(maxsize=None)
def threshold(kind, cdt, shapes=SMALL, accum=1, groups="driver"):
    """max_norm of the shared setup: the trajectory unclipped through graph=False -- code this feature leaves alone -- and the
    geometric mean of the smallest and largest fp64 norm of its flat gradients"""
    probe = trajectory(kind, cdt, False, None, shapes=shapes, accum=accum, groups=groups, by_hand=True)
    lo, hi = min(probe["flat64"]), max(probe["flat64"])
    print("%s %s unclipped norms %s -> max_norm %.6g" % (kind, cdt, ["%.5g" % x for x in probe["flat64"]], math.sqrt(lo * hi)))
    assert hi > 1.5 * lo
    return f32(math.sqrt(lo * hi))


@functools.lru_cache(maxsize=None)
def unfused(kind, cdt, shapes=SMALL, accum=1, groups="driver", by_hand=False, change=None):
    """the yardstick run: graph=False with the shared setup's max_grad_norm"""
    return trajectory(kind, cdt, False, threshold(kind, cdt, shapes, accum, groups), shapes=shapes, accum=accum, groups=groups, by_hand=by_hand, change=change)


def same_bits(run, ref, what):
    for k in ("p", "m", "v", "shadow", "logits"):
        assert torch.equal(run[k], ref[k]), "%s: %s differs, max %.3e" % (what, k, float((run[k].float() - ref[k].float()).abs().max()))
    assert run["gmax"] == 0.0 and ref["gmax"] == 0.0, what
    assert run["clip"] == ref["clip"], (what, run["clip"], ref["clip"])


def clipped_and_not(clip):
    coefs = [c for _, c in clip]
    assert any(c == 1.0 for c in coefs) and any(c < 1.0 for c in coefs), clip


def check_coefs(clip, norms64, max_norms):
    """the recorded (norm, coef) of every update against fp64 norms: the operator test's bounds"""
    assert len(clip) == len(norms64)
    for (norm, coef), n64, mx in zip(clip, norms64, max_norms):
        want = min(1.0, mx / (n64 + 1e-6))
        print("update: norm %.9g (fp64 over the .grad tensors %.9g) coef %.9g (fp64 %.9g)" % (norm, n64, coef, want))
        assert abs(norm - n64) <= 1e-6 * n64, (norm, n64)
        # (the engine's coefficient is formed from its own double norm, which is within ~1e-13 of n64)
        assert abs(coef - float(np.float32(want))) <= float(np.spacing(np.float32(want))), (coef, want)


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float32])
def test_clipped_fused_step_equals_the_unfused_path_bit_for_bit(kind, cdt):
    """four updates over two shapes: the replayed graph and the prologue + eager launches end p, m, v, the shadow and the eval logits on
    the bits of graph=False with the same max_grad_norm, and report the same (norm, coef) at every update.  Two captures for two
    shapes; max_grad_norm changed by hand before the third update adds none: the value travels with the step prologue."""
    mx = threshold(kind, cdt)
    change = (2, f32(0.7 * mx))
    ref = unfused(kind, cdt, change=change)
    graph = trajectory(kind, cdt, True, mx, change=change)
    eager = trajectory(kind, cdt, 2, mx, change=change)
    assert ref["stats"] == (0, 0) and graph["stats"] == (2, 4) and eager["stats"] == (0, 0), (ref["stats"], graph["stats"], eager["stats"])
    same_bits(graph, ref, "graph")
    same_bits(eager, ref, "prologue + eager launches")
    clipped_and_not(graph["clip"])
    assert all(u[:2] == (0, graph["n"]) for u in graph["update"]), graph["update"]
    # and the option does something: the unclipped run ends elsewhere
    plain = trajectory(kind, cdt, True, None)
    assert not torch.equal(plain["m"], graph["m"]) and plain["clip"] == []


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_engine_norm_is_the_fp64_norm_of_the_grad_tensors(kind):
    """at every update the engine's grad_clip_stats()[0] equals, to 1e-6, the fp64 norm over the named parameters' `.grad` tensors of the
    twin unfused model read after training_step() -- the tensors, not the flat buffer, so a writer that leaves something in the
    alignment padding between tensors shows up -- and coef is the operator's.  (Deterministic mode: the twin's gradients are the fused
    step's bit for bit, so the bound is about the norm alone.)"""
    cdt = torch.bfloat16
    mx = threshold(kind, cdt)
    twin = unfused(kind, cdt, by_hand=True)
    run = trajectory(kind, cdt, True, mx)
    same_bits(run, twin, "graph against the twin")
    for a, b in zip(twin["flat64"], twin["tensor64"]):
        assert abs(a - b) <= 1e-10 * b, ("the flat range holds more than the tensors", a, b)
    check_coefs(run["clip"], twin["tensor64"], [mx] * 4)
    check_coefs(twin["clip"], twin["tensor64"], [mx] * 4)
    clipped_and_not(run["clip"])


@pytest.mark.parametrize("mode", [True, False])
@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_moments_scale_with_the_coefficient(kind, mode):
    """one update from zero moments, twin models: clipping off, and max_norm = norm / 4.  m_clip = coef * m_off and v_clip = coef^2 *
    v_off elementwise to 1e-6 (a handful of fp32 roundings each, 6e-8 apiece), on the elements with |m_off| > 1e-20 (out of the
    denormals).  Through the graph, and through graph=False, which ties the Python-driven path to the formula on its own."""
    cdt = torch.bfloat16
    off = trajectory(kind, cdt, mode, None, nsteps=1)
    norm = unfused_first_norm(kind, cdt)
    on = trajectory(kind, cdt, mode, f32(norm / 4), nsteps=1)
    (got_norm, coef), = on["clip"]
    assert abs(got_norm - norm) <= 1e-6 * norm and 0.2 < coef < 0.3, (got_norm, norm, coef)
    n = on["n"]
    m_off, v_off = off["m"][:n].double(), off["v"][:n].double()
    m_on, v_on = on["m"][:n].double(), on["v"][:n].double()
    keep = m_off.abs() > 1e-20
    assert int(keep.sum()) > n // 4
    c = float(np.float32(coef))
    em = ((m_on - c * m_off).abs() / m_off.abs())[keep]
    ev = ((v_on - c * c * v_off).abs() / v_off)[keep]
    print("%s mode %s: coef %.9g, %d elements, worst relative error m %.3e v %.3e" % (kind, mode, coef, int(keep.sum()), float(em.max()), float(ev.max())))
    assert float(em.max()) <= 1e-6 and float(ev.max()) <= 1e-6


@functools.lru_cache(maxsize=None)
def unfused_first_norm(kind, cdt):
    return trajectory(kind, cdt, False, None, nsteps=1, by_hand=True)["tensor64"][0]


def test_clipping_the_accumulated_gradient():
    """accum = 2: the clipped quantity is the gradient accumulated over the window, and the bits are graph=False's"""
    kind, cdt, shapes = "bert", torch.bfloat16, ((5, 40),)
    mx = threshold(kind, cdt, shapes, 2)
    ref = unfused(kind, cdt, shapes, 2, by_hand=True)
    run = trajectory(kind, cdt, True, mx, shapes=shapes, accum=2)
    same_bits(run, ref, "accumulation")
    assert run["stats"] == (2, 8)                                                  # one graph with the update, one without
    check_coefs(run["clip"], ref["tensor64"], [mx] * 4)
    clipped_and_not(run["clip"])


def test_clipping_with_update_classes():
    kind, cdt = "bert", torch.bfloat16
    mx = threshold(kind, cdt, groups="classed")
    ref = unfused(kind, cdt, groups="classed")
    run = trajectory(kind, cdt, True, mx, groups="classed")
    same_bits(run, ref, "classed")
    clipped_and_not(run["clip"])
    assert all(u[2] > 2 and u[:2] == (0, run["n"]) for u in run["update"]), run["update"]


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_no_riders_under_clipping(kind):
    """B = 24, L = 50, where the backward launches carry riders: without clipping ridden > 0 as ever; with clipping no parameter moves
    before the whole gradient exists -- (ridden, swept) == (0, n_update_end); an optimizer without the option on the same model gets
    its riders back."""
    with env(MB_DETERMINISTIC=1, MB_GROUP_WGRAD=256, MB_ADAMW_RIDE=1):
        m = build(kind, 3, torch.bfloat16).train()
        core = m._core
        n = core.n_update_end
        seen = []
        with m.stream_scope():
            for i, mx in enumerate((None, 1.0, None)):
                opt = AdamW(optimizer_grouped_parameters(m), lr=LR, max_grad_norm=mx)
                m.train_step(*batch(kind, 24, 50, 90 + i), optimizer=opt, graph=True)
                seen.append(core.update_stats()[:2])
                if mx is None:
                    with pytest.raises(_lib.MagbertError):
                        core.grad_clip_stats()
                    assert opt.last_grad_norm is None
                else:
                    assert math.isfinite(opt.last_grad_norm) and opt.last_grad_norm > 0.0
        torch.cuda.synchronize()
    print("%s riders at T = 1200: %s of %d" % (kind, seen, n))
    assert seen[0][0] > 0 and sum(seen[0]) == n
    assert seen[1] == (0, n)
    assert seen[2] == seen[0]


# per-tensor bound of the oracle case = RATIO * the tensor's own peak group lr: the project's bound for this comparison
# (test_param_groups_gpu.py: test_three_classed_updates_track_the_oracle_fp32)
RATIO = 2e-4 / 1e-3


@functools.lru_cache(maxsize=None)
def oracle_run(kind):
    """three classed updates of the CPU oracle model with torch.nn.utils.clip_grad_norm_ in front of optim_ref.AdamW.step(); the labels of
    the second step times 8; max_norm = twice the norm of the first step's gradient (so that step is not clipped)"""
    layers = 2
    if kind == "bert":
        o = R.MAG_BertForSequenceClassification(R.BertConfigLite(num_hidden_layers=layers), R.MultimodalConfig(1.0, 0.0), 47, 74)
        o = R.set_dropout(R.load_deterministic(o, "test"), 0.0, 0.0, 0.0).train()
    else:
        o = X.MAG_XLNetForSequenceClassification(X.XLNetConfigLite(n_layer=layers), X.MultimodalConfig(1.0, 0.0), 47, 74)
        o = X.set_dropout(X.load_deterministic(o, "test"), 0.0, 0.0).train()
    ogroups = layerwise_lr_groups(o.named_parameters(), layers, LR, layer_decay=DECAY, head_lr=HEAD)
    peak = {}
    for g in ogroups:
        for p in g["params"]:
            peak[id(p)] = g["lr"]
    oo = O.AdamW(ogroups, lr=LR)
    so = O.get_linear_schedule_with_warmup(oo, num_warmup_steps=1.0, num_training_steps=10)
    mx, norms = None, []
    for s in range(3):
        i2, v2, a2, m2, s2, l2 = batch(kind, 4, 50, 50 + s, "cpu", label_mult=8.0 if s == 1 else 1.0)
        oo.zero_grad()
        torch.nn.functional.mse_loss(o(i2, v2, a2, m2, s2)[0].view(-1), l2.view(-1)).backward()
        if mx is None:
            mx = f32(2.0 * float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in o.parameters() if p.grad is not None))))
        norms.append(float(torch.nn.utils.clip_grad_norm_(o.parameters(), mx)))
        oo.step(); so.step()
    o.eval()
    i2, v2, a2, m2, s2, _ = batch(kind, 4, 50, 60, "cpu")
    with torch.no_grad():
        logits = o(i2, v2, a2, m2, s2)[0]
    params = {n: (p.detach().clone(), peak[id(p)], p.grad is not None) for n, p in o.named_parameters()}
    return params, logits, mx, norms


def against_oracle(kind, mode):
    params, logits0, mx, _ = oracle_run(kind)
    layers = 2
    m = build(kind, layers, torch.float32, dropout=False).train()
    opt = AdamW(layerwise_lr_groups(m.named_parameters(), layers, LR, layer_decay=DECAY, head_lr=HEAD), lr=LR, max_grad_norm=mx)
    sch = get_linear_schedule_with_warmup(opt, num_warmup_steps=1.0, num_training_steps=10)
    clip = []
    for s in range(3):
        m.train_step(*batch(kind, 4, 50, 50 + s, label_mult=8.0 if s == 1 else 1.0), optimizer=opt, graph=mode)
        sch.step()
        clip.append(opt.last_grad_clip)
    torch.cuda.synchronize()
    rows = []
    for n, p in m.named_parameters():
        want, lr, trained = params[n]
        if not trained:
            assert torch.equal(p.detach().cpu(), want), n
            continue
        rows.append((float((p.detach().cpu() - want).abs().max()) / (RATIO * lr), n))
    m.eval()
    data = batch(kind, 4, 50, 60)
    with torch.no_grad():
        l1 = m(data[0], data[1], data[2], token_type_ids=data[4], attention_mask=data[3])[0].cpu()
    return rows, float((l1 - logits0).abs().max()), clip, m


@pytest.mark.parametrize("kind", ["bert", "xlnet"])
def test_three_clipped_updates_track_the_oracle_fp32(kind):
    """fp32, dropout off, two layers, three classed updates through the replayed graph against oracle.optim_ref.AdamW with
    torch.nn.utils.clip_grad_norm_(o.parameters(), max_norm) on the CPU oracle model: every tensor within RATIO * its group's peak
    learning rate, eval logits within 5e-3 -- the existing bound of test_three_classed_updates_track_the_oracle_fp32; the coefficient
    adds about 1e-6 relative.  The same comparison through graph=False is printed next to it.  Measured, worst tensor as a fraction of
    its bound (the word-embedding table every time): MAG-BERT unfused 0.024, fused 0.024; MAG-XLNet unfused 0.011, fused 0.011."""
    _, _, mx, onorms = oracle_run(kind)
    rows_u, logit_u, clip_u, _ = against_oracle(kind, False)
    rows_f, logit_f, clip_f, m = against_oracle(kind, True)
    wu, wf = max(rows_u), max(rows_f)
    print("%s clipped oracle case (max_norm %.5g, oracle norms %s, fused (norm, coef) %s): worst err / bound unfused %.3f (%s), fused %.3f (%s); "
          "logits %.2e / %.2e" % (kind, mx, ["%.5g" % x for x in onorms], clip_f, wu[0], wu[1], wf[0], wf[1], logit_u, logit_f))
    assert m._core.update_stats()[2] > 2 and m._core.graph_stats() == (1, 3)
    clipped_and_not(clip_f)
    for (norm, _), on in zip(clip_f, onorms):
        assert abs(norm - on) <= 1e-3 * on, (clip_f, onorms)          # (a sanity check: two fp32 implementations of one gradient)
    bad = [(r, n) for r, n in rows_f if r > 1.0]
    assert not bad and logit_f <= 5e-3, (bad, logit_f)
    assert wu[0] <= 1.0 and logit_u <= 5e-3, (wu, logit_u)


@pytest.mark.parametrize("model", ["bert-base-uncased", "xlnet-base-cased"])
def test_driver_epoch_with_max_grad_norm(model):
    """--synthetic 96 --n_epochs 1 --max_grad_norm 1.0: runs, a finite loss, and every update went through the single call"""
    from bert_multimodal_transformer_amd import multimodal_driver as D
    old = getattr(D, "args", None)
    try:
        D.args = D.parse_args(["--model", model, "--synthetic", "96", "--n_epochs", "1", "--max_grad_norm", "1.0", "--seed", "5"])
        D.set_random_seed(D.args.seed)
        tr, dev, te, nsteps = D.set_up_data_loader()
        m, opt, sch = D.prep_for_training(nsteps)
        assert opt.max_grad_norm == 1.0
        loss = D.train_epoch(m, tr, opt, sch)
        torch.cuda.synchronize()
        captures, launches = m._core.graph_stats()
        norm, coef = m._core.grad_clip_stats()
        print("%s: train loss %.4f, %d graph launches, last norm %.4g coef %.4g" % (model, loss, launches, norm, coef))
        assert np.isfinite(loss) and launches > 0 and np.isfinite(norm) and 0.0 < coef <= 1.0
        assert opt.last_grad_norm == norm
    finally:
        D.args = old
