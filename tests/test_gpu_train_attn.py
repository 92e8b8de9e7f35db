"""The fused attention operator of the training path (`vog_attn_fused_f32`, csrc/train_attn.hip) on the device: against torch
autograd on the CPU in fp32, against the materialised operator (`vog_attn_f32`) under dropout, against the rounded-operand
restatement under amp, and through the trainer / autograd path with `attn="fused"`. Every operator call runs on a scratch of
exactly `vog_attn_fused_scratch_bytes` between two guard bands, at both shifts of the base."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_amp import _ACC, _attn_rounded, _check, _switch, MODES
from tests.test_gpu_bwd_ops import _attn_ref
from tests.test_gpu_train_ops import guarded

pytestmark = pytest.mark.gpu
bwd = importlib.import_module("vognet-pytorch_amd.backward")
L = bwd.L
TOL, TOL_SUM = 2e-5, 1e-4          # tests/test_gpu_bwd_ops.py: fp32 on both sides, another summation order
SHIFTS = (1, 252)
VW, VH, FDIV = 720.0, 405.0, 10.0
GRADS = ("d_x", "g_wq", "g_wk", "g_wv", "g_pe_w", "g_pe_b")


def close(a, b, tol=TOL, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double().reshape(a.shape)
    scale = max(float(b.abs().max()), 1e-12)
    err = float((a - b).abs().max()) / scale
    print(f"    {what}: {err:.3e} (bound {tol:.0e})")
    assert err <= tol, (what, err)
    return err


def fused_call(w, pe, x, S, N, n, H, boxes, shift=1, **kw):
    with guarded(L.load().vog_attn_fused_scratch_bytes(S, N, n, x.shape[1], H), 8, shift) as sc:
        return bwd._attn_call(w, pe, x, S, N, n, H, boxes, scratch=sc, fused=True, **kw)


@functools.lru_cache(maxsize=None)
def _case(S, n, nsrl, d, H, rel, wscale=1.0):
    """Inputs and the CPU autograd reference of one geometry, computed once and shared (treated as read-only)."""
    g = torch.Generator().manual_seed(S * 1000 + n * 10 + d)
    N = n * nsrl
    x = torch.randn(S, N, d, generator=g)
    ws = [torch.randn(d, d, generator=g) / math.sqrt(d) for _ in range(3)]
    ws[0], ws[1] = ws[0] * wscale, ws[1] * wscale
    props = torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])
    pe_w, pe_b = torch.randn(H, 5, generator=g), torch.randn(H, generator=g) * 0.3
    d_cat = torch.randn(S, N, d, generator=g)
    bx = (props[:, :5] / torch.tensor([VW, VH, VW, VH, FDIV])).reshape(S, n, 5) if rel else None
    c = dict(S=S, n=n, N=N, d=d, H=H, rel=rel, x=x, ws=ws, props=props, pe_w=pe_w, pe_b=pe_b, d_cat=d_cat, bx=bx, nsrl=nsrl)
    lv = [t.clone().requires_grad_(True) for t in [x] + ws + [pe_w, pe_b]]
    cat = _attn_ref(lv[0], lv[1], lv[2], lv[3], bx, lv[4], lv[5], H, nsrl)
    (cat * d_cat).sum().backward()
    c["ref"] = dict(cat=cat.detach(), d_x=lv[0].grad, g_wq=lv[1].grad, g_wk=lv[2].grad, g_wv=lv[3].grad,
                    g_pe_w=lv[4].grad if rel else None, g_pe_b=lv[5].grad if rel else None)
    return c


def _dev(c):
    w = {"wq": c["ws"][0].cuda(), "wk": c["ws"][1].cuda(), "wv": c["ws"][2].cuda()}
    boxes = bwd._Boxes(c["props"].cuda(), VW, VH, FDIV) if c["rel"] else None
    pe = (c["pe_w"].cuda(), c["pe_b"].cuda()) if c["rel"] else None
    xd = c["x"].reshape(c["S"] * c["N"], c["d"]).cuda().contiguous()
    dc = c["d_cat"].reshape(c["S"] * c["N"], c["d"]).cuda().contiguous()
    return (w, pe, xd, c["S"], c["N"], c["n"], c["H"], boxes), dc


def _against_ref(c, shift):
    args, dc = _dev(c)
    f = fused_call(*args, shift=shift)
    r = fused_call(*args, shift=shift, d_cat=dc)
    torch.cuda.synchronize()
    ref = c["ref"]
    close(f["cat"], ref["cat"], what="cat")
    for k in GRADS:
        if ref[k] is not None:
            close(r[k], ref[k], tol=TOL_SUM if "pe" in k else TOL, what=k)
    return f, r


SHAPES = [(2, 1, 1, 8, 2, True), (3, 7, 1, 32, 3, True), (2, 5, 3, 48, 3, True), (1, 9, 2, 20, 4, False), (5, 33, 1, 64, 8, True),
          (2, 65, 1, 64, 2, True), (3, 100, 1, 512, 3, True), (2, 20, 5, 768, 3, True), (1, 300, 1, 96, 3, True)]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("S,n,nsrl,d,H,rel", SHAPES)
def test_fused_f32_vs_cpu_autograd(S, n, nsrl, d, H, rel, shift):
    _against_ref(_case(S, n, nsrl, d, H, rel), shift)


def test_fused_f32_row_maxima_move_between_key_tiles():
    """wq, wk * 8: sharp rows whose maximum lies in late key tiles for some rows and early ones for others, so the running
    maximum and sum of the online softmax are rescaled on the way (checked on the CPU reference first)."""
    c = _case(1, 300, 1, 96, 3, True, 8.0)
    q, k = c["x"] @ c["ws"][0].t(), c["x"] @ c["ws"][1].t()
    diff = c["bx"].unsqueeze(2) - c["bx"].unsqueeze(1)
    for h in range(3):
        lg = q[..., 32 * h:32 * h + 32] @ k[..., 32 * h:32 * h + 32].transpose(1, 2) + torch.relu(diff @ c["pe_w"][h] + c["pe_b"][h])
        am = lg.argmax(-1).flatten()
        late, early = float((am >= 200).float().mean()), float((am < 100).float().mean())
        print(f"    head {h}: row maximum in the last third {late:.2f}, in the first third {early:.2f}")
        assert late >= 0.25 and early >= 0.25, (h, late, early)
    _against_ref(c, 1)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("shape", [(2, 5, 3, 48, 3, True), (2, 65, 1, 64, 2, True), (1, 9, 2, 20, 4, False)])
@pytest.mark.parametrize("drop", [None, (0.2, 77, 210)])
def test_standalone_backward_equals_kept_forward_backward(shape, drop, shift):
    c = _case(*shape)
    args, dc = _dev(c)
    f = fused_call(*args, shift=shift, drop=drop)
    assert f["lse"].shape == (c["S"], c["H"], c["N"])
    alone = fused_call(*args, shift=shift, d_cat=dc, drop=drop)
    kept = fused_call(*args, shift=shift, d_cat=dc, drop=drop, lse=f["lse"], cat=f["cat"])
    again = fused_call(*args, shift=shift, d_cat=dc, drop=drop)
    torch.cuda.synchronize()
    for k in GRADS:
        if k in alone:
            assert torch.equal(alone[k], kept[k]), k
            assert torch.equal(alone[k], again[k]), k                      # two identical calls: identical bits
    f2 = fused_call(*args, shift=shift, drop=drop)
    assert torch.equal(f["cat"], f2["cat"]) and torch.equal(f["lse"], f2["lse"])


@pytest.mark.parametrize("shift", SHIFTS)
def test_options(shift):
    c = _case(2, 5, 3, 48, 3, True)
    args, dc = _dev(c)
    full = fused_call(*args, shift=shift, d_cat=dc)
    for skip in ("wq", "wk", "wv", "pe", "dx"):
        want = {"wq", "wk", "wv", "pe"} - {skip}
        r = fused_call(*args, shift=shift, d_cat=dc, want=want, want_dx=skip != "dx")
        torch.cuda.synchronize()
        gone = {"wq": ["g_wq"], "wk": ["g_wk"], "wv": ["g_wv"], "pe": ["g_pe_w", "g_pe_b"], "dx": ["d_x"]}[skip]
        for k in GRADS:
            if k in gone:
                assert k not in r
            else:
                assert torch.equal(r[k], full[k]), (skip, k)
    base = torch.randn(full["d_x"].shape, generator=torch.Generator().manual_seed(5)).cuda()
    r = fused_call(*args, shift=shift, d_cat=dc, d_x=base.clone(), accumulate_dx=True)
    torch.cuda.synchronize()
    # base + the three products against the three products summed first: three fp32 additions on either side, each within
    # half a unit (2^-24) of the result's size
    close(r["d_x"], base.double() + full["d_x"].double(), tol=6 * 2.0 ** -24, what="accumulated d_x")


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("shape", [(2, 5, 3, 48, 3, True), (2, 65, 1, 64, 2, True), (3, 100, 1, 512, 3, True)])
def test_dropout_masks_are_the_materialised_operators(shape, shift):
    c = _case(*shape)
    args, dc = _dev(c)
    drop = (0.2, 12345, 120)
    m_f = bwd._attn_call(*args, drop=drop)
    m_b = bwd._attn_call(*args, d_cat=dc, drop=drop)
    f = fused_call(*args, shift=shift, drop=drop)
    r = fused_call(*args, shift=shift, d_cat=dc, drop=drop)
    torch.cuda.synchronize()
    close(f["cat"], m_f["cat"], what="cat")
    for k in GRADS:
        close(r[k], m_b[k], tol=TOL_SUM if "pe" in k else TOL, what=k)


@pytest.mark.parametrize("shift", SHIFTS)
def test_dropout_zero_fraction_with_one_key(shift):
    """N = 1: every row has one probability, 1, so a dropped element is an exactly-zero row of a head's output."""
    c = _case(64, 1, 1, 8, 2, True)
    args, dc = _dev(c)
    drop = (0.2, 4242, 110)
    m_f = bwd._attn_call(*args, drop=drop)
    f = fused_call(*args, shift=shift, drop=drop)
    torch.cuda.synchronize()
    zf, zm = (f["cat"] == 0), (m_f["cat"] == 0)
    print(f"    exactly-zero outputs: fused {int(zf.sum())}, materialised {int(zm.sum())} of {zf.numel()}")
    assert torch.equal(zf, zm) and 0 < int(zf.sum()) < zf.numel()
    close(f["cat"], m_f["cat"], what="cat")


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("S,n,nsrl,d,H", [(2, 20, 1, 512, 3), (3, 7, 2, 32, 3), (2, 65, 1, 64, 2)])
def test_fused_amp_vs_rounded_restatement(S, n, nsrl, d, H, mode):
    """`_check` prints every deviation (recorded in profiles/amp_kernel_deviations.txt under the fused operator's heading)."""
    dt, amp = MODES[mode]
    c = _case(S, n, nsrl, d, H, True)

    def restate():
        lv = [t.clone().requires_grad_(True) for t in [c["x"]] + c["ws"] + [c["pe_w"], c["pe_b"]]]
        cat = _attn_rounded(lv[0], lv[1], lv[2], lv[3], c["bx"], lv[4], lv[5], H, nsrl, dt)
        (cat * c["d_cat"]).sum().backward()
        return cat.detach(), [t.grad for t in lv]

    cat, grads = restate()
    _ACC[0] = torch.float64
    try:
        alt_cat, alt = restate()
    finally:
        _ACC[0] = torch.float32
    args, dc = _dev(c)
    lib = L.load()
    assert lib.vog_train_set_int(b"amp", amp) == 0 and lib.vog_train_set_int(b"f32_products", 0) == 0
    try:
        f = fused_call(*args)
        r = fused_call(*args, d_cat=dc, shift=252)
        torch.cuda.synchronize()
        assert _switch(b"f32_products") == 0              # uneven heads too: no fp32 product launch
    finally:
        lib.vog_train_set_int(b"amp", 0)
    case = f"fused attn S={S} N={n * nsrl} d={d} H={H}"
    _check(mode, f["cat"], cat, alt_cat, f"{case} cat")
    got = [r["d_x"].reshape(S, n * nsrl, d), r["g_wq"], r["g_wk"], r["g_wv"], r["g_pe_w"], r["g_pe_b"]]
    for i, k in enumerate(("d_x", "wq", "wk", "wv", "pe_w", "pe_b")):
        _check(mode, got[i], grads[i], alt[i], f"{case} {k}")


# ---------------------------------------------------------------- the whole path: trainer, autograd, Learner's options
from tests.gpu_util import comm_for                                         # noqa: E402
from tests.test_gpu_amp import _compare, _sd                                # noqa: E402
from tests.test_gpu_autograd import _build, _close, _grads                  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
cases = importlib.import_module("oracle.cases")
mgb = importlib.import_module("oracle.make_golden_bwd")


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep_cmpmsk", "full/cfg2_vog_spat_gt5_bs4"])
def test_trainer_fused_vs_reference_golden_and_materialised(name):
    """Bounds: tests/test_gpu_surface.py::test_device_training_steps_vs_oracle_adam's for the trainer's own forward (loss 2e-5,
    mdl_outs 1e-4, gradients 5e-3 of the largest reference entry); against the materialised trainer 2e-5 per tensor."""
    from tests.test_bwd_oracle import check_fixture
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    tf = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, attn="fused")
    tm = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    assert tm.attn == "materialized"
    g = np.load(mgb.bwd_path(name))
    lf, gf = tf.gradients(dev)
    lm, gm = tm.gradients(dev)
    assert abs(float(lf["loss"]) - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    ref_outs = torch.from_numpy(np.load(cases.golden_path(name))["mdl_outs"])
    outs = tf.forward(dev)[0]["mdl_outs"].cpu()
    assert float((outs - ref_outs).abs().max()) <= 1e-4 * float(ref_outs.abs().max())
    worst = max(check_fixture(g, "p:" + k, v.cpu().numpy(), tol=5e-3) for k, v in gf.items())
    assert len(gf) == sum(1 for k in g.files if k.startswith("p:") and k.endswith("__shape"))
    assert set(gf) == set(gm)
    assert abs(float(lf["loss"]) - float(lm["loss"])) <= 2e-5 * abs(float(lm["loss"]))
    wm = max(_close(gf[k], gm[k].cpu(), 2e-5, k) for k in gm)
    print(f"    {name}: worst against the golden {worst:.3e}, against the materialised trainer {wm:.3e}")


def test_three_adam_steps_follow_the_materialised_path():
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    tf = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, attn="fused")
    tm = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    a = [float(tf.step(dev)["loss"]) for _ in range(3)]
    b = [float(tm.step(dev)["loss"]) for _ in range(3)]
    print("    losses fused", a, "materialised", b)
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-5 * abs(y), (a, b)


def test_autograd_path_takes_the_operator_from_the_cfg(monkeypatch):
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    cfg.hip.train_attn = "fused"
    calls = []
    orig = bwd._attn_call
    monkeypatch.setattr(bwd, "_attn_call", lambda *a, **k: (calls.append(bool(k.get("fused"))), orig(*a, **k))[1])
    tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, attn="fused")
    _, ref = tr.gradients(dev)
    mdl.eval().requires_grad_(True)
    loss_fn(mdl(dev), dev)["loss"].backward()
    assert calls and all(calls)                               # every attention call of both paths went to the fused entry
    got = _grads(mdl)
    assert set(got) == set(ref)
    for k, v in ref.items():
        _close(got[k], v.cpu(), 1e-6, k)


def test_train_mode_dropout_step_in_amp_bf16():
    """tests/test_gpu_amp.py::test_amp_train_mode_dropout_close_to_fp32's criterion, both trainers fused."""
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    kw = dict(lr=1e-4, dropout=True, dropout_seed=7, attn="fused")
    t32 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, **kw)
    t16 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, amp="bf16", **kw)
    l32, g32 = t32.gradients(dev)
    l16, g16 = t16.gradients(dev)
    e32, _ = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, attn="fused").gradients(dev)
    assert abs(float(l32["loss"]) - float(e32["loss"])) > 1e-6 * abs(float(e32["loss"]))     # the masks are on
    assert abs(float(l16["loss"]) - float(l32["loss"])) <= 1e-3 * abs(float(l32["loss"]))
    worst, cos_min, differs = _compare(g32, g16, "fused train mode bf16")
    assert differs and worst <= 0.2 and cos_min >= 0.99, (worst, cos_min)
    assert math.isfinite(float(t16.step(dev)["loss"]))


def test_default_does_not_reach_the_fused_operator(monkeypatch):
    """Three fp32 steps with the option left out against three with "materialized" spelled out, while both entries of the new
    file raise when called: parameters and Adam moments byte-equal, every attention call the materialised one, no geometry
    key for the backward. (Bit-equality with the parent commit's package: scratch/time_train_attn.py, profiles/train_attn.json.)"""
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    lib = L.load()
    seen = []
    orig = bwd._attn_call
    monkeypatch.setattr(bwd, "_attn_call", lambda *a, **k: (seen.append(k.get("fused", False)), orig(*a, **k))[1])

    def refuse(*a):
        raise AssertionError("the default step called the fused entry")

    monkeypatch.setattr(lib, "vog_attn_fused_f32", refuse)
    monkeypatch.setattr(lib, "vog_attn_fused_scratch_bytes", refuse)
    ta = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, attn="materialized")
    tb = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    for _ in range(3):
        ta.step(dev); tb.step(dev)
    torch.cuda.synchronize()
    assert seen and not any(seen)
    for k in ta.params:
        assert torch.equal(ta.params[k], tb.params[k]), k
    for k in ta.m:
        assert torch.equal(ta.m[k], tb.m[k]) and torch.equal(ta.v[k], tb.v[k]), k
    assert "attn_fused" not in ta._geo(dev)
