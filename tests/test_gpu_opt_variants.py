"""The optimiser variants on the device: vog_opt_step_ex_f32 (AdamW's decoupled decay, AMSGrad, maximize, grad_scale) and
vog_opt_accum_f32 (csrc/optim.hip), `FP32Trainer(optimizer=, amsgrad=, maximize=, accum_steps=)`, its state against torch's own
optimizers, and the Learner with the plateau scheduler and an accumulation window over an odd number of batches.

The seeded tensor set of tests/test_gpu_opt.py (under 1 M elements, 79 tensors: several launch tables; a quadruple with a scalar
head and one without a common alignment) with one more offset column for vmax: `XOFF` makes tensor 5 the case "vmax alone
disagrees" (one element per lane although p, g, m, v agree) and the scalar-head quadruple the case "five pointers agree".

Values are compared with torch.optim.Adam / AdamW themselves, in float64 on the CPU, one step at a time: before every step the
reference takes the device's fp32 state, so the bounds are those of ONE fp32 step (test_gpu_opt._check_mode_b's): m, v, vmax
1e-6 relative (m relative to |b1 m| + |(1 - b1) g|), |p - p_ref| <= 2^-23 |p| + 1e-4 lr, and 2^-22 |p| + 1e-4 lr where p is
rounded once more (decoupled decay; a gradient that was summed and scaled on the device)."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

from tests.gpu_util import comm_for
from tests.test_gpu_autograd import _build
from tests.test_gpu_opt import B1, B2, EPS, LR, MIS, NAME, OFFSETS, SIZES, _dev, _host, _read, _same, _sd, _state

pytestmark = pytest.mark.gpu

trn = importlib.import_module("vognet-pytorch_amd.train")
L = importlib.import_module("vognet-pytorch_amd.lib")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")

XOFF = [0] * len(SIZES)                 # elements into the buffer: vmax
XOFF[5] = 2                             # p, g, m, v agree (16-byte accesses without vmax), vmax alone disagrees
XOFF[MIS] = 1                           # five pointers agree one element in: scalar head, then 16-byte accesses
VMAX_ALONE = 5
WD = float(np.float32(0.01))
SPLIT = 40                              # two groups: tensors [0, 40) with weight decay, [40, 79) without
GROUPS = [(0, SPLIT, LR, WD), (SPLIT, len(SIZES) - SPLIT, LR, 0.0)]
GUARD = 777.0


def _devx(host_list, offs=XOFF):
    """Device copies at the offsets `offs` -> (views, buffers); the elements around a view hold GUARD."""
    views, bufs = [], []
    for t, off in zip(host_list, offs):
        buf = torch.full((t.numel() + 4,), GUARD, dtype=torch.float32, device="cuda")
        view = buf[off:off + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * off
        views.append(view), bufs.append(buf)
    return views, bufs


def _guards_intact(bufs, offs, sizes=SIZES):
    return all(bool((b[:o] == GUARD).all()) and bool((b[o + n:] == GUARD).all()) for b, o, n in zip(bufs, offs, sizes))


def _fill(a, p, g, m, v, state, step, max_norm, growth):
    lib = L.load()
    arr = (L.OptTensor * len(p))()
    for i in range(len(p)):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = L.ptr(p[i]), L.ptr(g[i]), L.ptr(m[i]), L.ptr(v[i]), p[i].numel()
    a.tensors, a.n_tensors = arr, len(p)
    a.lr, a.beta1, a.beta2, a.eps, a.step = LR, B1, B2, EPS, step
    scratch = None
    if state is not None:
        scratch = torch.empty(int(lib.vog_opt_scratch_bytes(len(p), sum(t.numel() for t in p))), dtype=torch.uint8, device="cuda")
        a.state, a.scratch, a.scratch_bytes = L.ptr(state), L.ptr(scratch), scratch.numel()
        a.max_norm = max_norm
        a.growth_factor, a.backoff_factor, a.growth_interval = growth
    return arr, scratch


def _garr(groups):
    garr = (L.OptGroup * len(groups))()
    for i, (first, count, lr, wd) in enumerate(groups):
        garr[i].first, garr[i].count, garr[i].lr, garr[i].weight_decay = first, count, lr, wd
    return garr


def _groups_step(p, g, m, v, groups=GROUPS, state=None, step=1, max_norm=0.0, growth=(2.0, 0.5, 2000)):
    ga = L.OptGroupsArgs()
    keep = _fill(ga.base, p, g, m, v, state, step, max_norm, growth)
    garr = _garr(groups)
    ga.groups, ga.n_groups = garr, len(groups)
    L.check(L.load().vog_opt_step_groups_f32(C.byref(ga), L.stream_ptr()), "vog_opt_step_groups_f32")
    torch.cuda.synchronize()


def _ex_step(p, g, m, v, vmax=None, groups=GROUPS, flags=0, grad_scale=1.0, state=None, step=1, max_norm=0.0, growth=(2.0, 0.5, 2000)):
    ex = L.OptExArgs()
    keep = _fill(ex.groups.base, p, g, m, v, state, step, max_norm, growth)
    garr = _garr(groups)
    ex.groups.groups, ex.groups.n_groups = garr, len(groups)
    ex.flags, ex.grad_scale = flags, grad_scale
    if vmax is not None:
        vm = (C.c_void_p * len(p))()
        for i in range(len(p)):
            vm[i] = L.ptr(vmax[i])
        ex.vmax = vm
    L.check(L.load().vog_opt_step_ex_f32(C.byref(ex), L.stream_ptr()), "vog_opt_step_ex_f32")
    torch.cuda.synchronize()


def _zeros(h):
    return [torch.zeros_like(t) for t in h["p0"]]


# ---------------------------------------------------------------- bit identity
@pytest.mark.parametrize("mode_b", [False, True])
def test_ex_without_flags_is_the_grouped_step_bit_for_bit(mode_b):
    h = _host()
    a = [_dev(h["p0"], 0), _dev(_zeros(h), 2), _dev(_zeros(h), 3)]
    b = [_dev(h["p0"], 0), _dev(_zeros(h), 2), _dev(_zeros(h), 3)]
    sa = _state(scale=4.0) if mode_b else None
    sb = _state(scale=4.0) if mode_b else None
    for step in (1, 2, 3):
        g = _dev(h["gs"][step - 1], 1)
        _groups_step(*a[:1], g, *a[1:], state=sa, step=step, max_norm=1.0)
        _ex_step(*b[:1], g, *b[1:], state=sb, step=step, max_norm=1.0)
        for k in range(3):
            assert _same(a[k], b[k]), (step, k)
        if mode_b:
            assert torch.equal(sa.cpu(), sb.cpu()) and _read(sb).adam_step == step
    assert not _same(b[0], _dev(h["p0"], 0))


def test_grad_scale_and_maximize_are_exact_factors_of_the_gradient():
    """Mode A. grad_scale = 0.5 on 2 g is grad_scale = 1 on g (two values of the one apply kernel's factor), and maximize on
    -g is the plain step on g: powers of two and signs are exact."""
    h = _host()
    runs = []
    for factor, flags, scale in ((1.0, 0, 1.0), (2.0, 0, 0.5), (-1.0, L.OPT_MAXIMIZE, 1.0), (-4.0, L.OPT_MAXIMIZE, 0.25)):
        p, m, v = _dev(h["p0"], 0), _dev(_zeros(h), 2), _dev(_zeros(h), 3)
        for step in (1, 2, 3):
            g = _dev([x * factor for x in h["gs"][step - 1]], 1)
            _ex_step(p, g, m, v, flags=flags, grad_scale=scale, step=step)
        runs.append((p, m, v))
    for r in runs[1:]:
        for k in range(3):
            assert _same(runs[0][k], r[k]), k


# ---------------------------------------------------------------- values against torch.optim
def _torch_opt(h, decoupled, amsgrad, maximize):
    params = [torch.nn.Parameter(t.double().clone()) for t in h["p0"]]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": params[:SPLIT], "weight_decay": WD}, {"params": params[SPLIT:], "weight_decay": 0.0}], lr=LR,
              betas=(B1, B2), eps=EPS, amsgrad=amsgrad, maximize=maximize, foreach=False)
    return params, opt


def _load_ref(params, opt, p, m, v, vmax, step):
    """The device's fp32 state becomes the float64 reference's (torch's own state layout)."""
    for i, q in enumerate(params):
        q.data.copy_(p[i].cpu().double())
        st = opt.state[q]
        if not st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(q.data), torch.zeros_like(q.data)
            if vmax is not None:
                st["max_exp_avg_sq"] = torch.zeros_like(q.data)
        st["step"].fill_(float(step))
        st["exp_avg"].copy_(m[i].cpu().double())
        st["exp_avg_sq"].copy_(v[i].cpu().double())
        if vmax is not None:
            st["max_exp_avg_sq"].copy_(vmax[i].cpu().double())


def _compare(params, opt, p, m, v, vmax, terms, p_ulps, what):
    wm = wv = wx = wp = 0.0
    for i, q in enumerate(params):
        st = opt.state[q]
        rp, rm, rv = q.data, st["exp_avg"], st["exp_avg_sq"]
        wm = max(wm, float(((m[i].cpu().double() - rm).abs() / terms[i]).max()))
        wv = max(wv, float(((v[i].cpu().double() - rv).abs() / rv).max()))
        if vmax is not None:
            rx = st["max_exp_avg_sq"]
            wx = max(wx, float(((vmax[i].cpu().double() - rx).abs() / rx).max()))
        wp = max(wp, float(((p[i].cpu().double() - rp).abs() / (p_ulps * 2.0 ** -23 * rp.abs() + 1e-4 * LR)).max()))
    print(f"{what}: worst m {wm:.2e}, v {wv:.2e}, vmax {wx:.2e}, p error / bound {wp:.3f}")
    assert wm <= 1e-6 and wv <= 1e-6 and wx <= 1e-6, (what, wm, wv, wx)
    assert wp <= 1.0, (what, wp)


@pytest.mark.parametrize("decoupled, amsgrad, maximize", [(True, False, False), (False, True, False), (True, True, False),
                                                          (False, False, True)],
                         ids=["adamw", "amsgrad", "amsgrad+adamw", "maximize"])
def test_three_steps_against_torch_optim_in_float64(decoupled, amsgrad, maximize):
    """Mode A, two groups (weight decay 0.01 / 0). The third step's gradients are multiplied by 0.1 (on both sides): v then
    falls below its running maximum in most entries, so the step is taken with vmax, not with v."""
    h = _host()
    flags = (L.OPT_DECOUPLED if decoupled else 0) | (L.OPT_AMSGRAD if amsgrad else 0) | (L.OPT_MAXIMIZE if maximize else 0)
    p, m, v = _dev(h["p0"], 0), _dev(_zeros(h), 2), _dev(_zeros(h), 3)
    vmax, xbufs = _devx(_zeros(h)) if amsgrad else (None, None)
    params, opt = _torch_opt(h, decoupled, amsgrad, maximize)
    for step in (1, 2, 3):
        gs = [x * (0.1 if step == 3 else 1.0) for x in h["gs"][step - 1]]
        _load_ref(params, opt, p, m, v, vmax, step - 1)
        terms = []
        for i, q in enumerate(params):
            q.grad = gs[i].double()
            wd = WD if (i < SPLIT and not decoupled) else 0.0                   # (L2 decay is part of the gradient the moments see)
            sign = -1.0 if maximize else 1.0
            terms.append((B1 * opt.state[q]["exp_avg"]).abs() + ((1 - B1) * (sign * q.grad + wd * q.data)).abs())
        opt.step()
        _ex_step(p, _dev(gs, 1), m, v, vmax=vmax, flags=flags, step=step)
        _compare(params, opt, p, m, v, vmax, terms, 2.0 if decoupled else 1.0, f"step {step}")
    if amsgrad:
        assert _guards_intact(xbufs, XOFF)
        above = [opt.state[q]["max_exp_avg_sq"] > opt.state[q]["exp_avg_sq"] for q in params]
        share = sum(int(a.sum()) for a in above) / sum(SIZES)
        print(f"entries with vmax > v after step 3: {share:.3f}")
        assert share >= 0.5, share
        for i, a in enumerate(above):
            assert bool((vmax[i].cpu() != v[i].cpu())[a].all()), i
        assert bool((vmax[VMAX_ALONE] >= v[VMAX_ALONE]).all()) and bool((vmax[MIS] >= v[MIS]).all())


def test_mode_b_with_amsgrad_clips_the_averaged_gradient():
    """max_norm = 1, amsgrad, grad_scale = 0.5 on gradients 2 g: the statistics see g (what clip_grad_norm_ would see),
    whatever the sign. Reference: clip_grad_norm_ + torch.optim.Adam(amsgrad=True) in float64 from the fp32 state after two
    steps, with vmax = 1.5 v there."""
    h = _host()
    gs = h["gs"][2]
    x0 = [t * 1.5 for t in h["v"]]
    for flags in (L.OPT_AMSGRAD, L.OPT_AMSGRAD | L.OPT_MAXIMIZE):
        p, m, v = _dev(h["p"], 0), _dev(h["m"], 2), _dev(h["v"], 3)
        vmax, xbufs = _devx(x0)
        params, opt = _torch_opt(h, False, True, bool(flags & L.OPT_MAXIMIZE))
        _load_ref(params, opt, p, m, v, vmax, 2)
        for i, q in enumerate(params):
            q.grad = gs[i].double()
        norm = float(torch.nn.utils.clip_grad_norm_(params, 1.0))
        coef = min(1.0, 1.0 / (norm + 1e-6))
        terms = []
        for i, q in enumerate(params):
            wd = WD if i < SPLIT else 0.0
            sign = -1.0 if flags & L.OPT_MAXIMIZE else 1.0
            terms.append((B1 * opt.state[q]["exp_avg"]).abs() + ((1 - B1) * (sign * q.grad + wd * q.data)).abs())
        opt.step()
        st = _state(scale=1.0, tracker=7, adam_step=2)
        _ex_step(p, _dev([x * 2.0 for x in gs], 1), m, v, vmax=vmax, flags=flags, grad_scale=0.5, state=st, max_norm=1.0)
        s = _read(st)
        assert s.found_inf == 0 and s.adam_step == 3 and s.skipped == 0 and s.growth_tracker == 8 and s.scale == 1.0
        e_norm, e_coef = abs(s.grad_norm - norm) / norm, abs(s.coef - coef) / coef
        print(f"flags {flags}: grad_norm {s.grad_norm} (ref {norm}) rel {e_norm:.2e}, coef {s.coef} rel {e_coef:.2e}")
        assert e_norm <= 1e-5 and e_coef <= 1e-5 and s.coef < 1.0, (e_norm, e_coef)
        _compare(params, opt, p, m, v, vmax, terms, 1.0, f"mode B, flags {flags}")
        assert _guards_intact(xbufs, XOFF)


# ---------------------------------------------------------------- overflow
def test_overflow_with_amsgrad_writes_nothing():
    h = _host()
    p, g, m, v = _dev(h["p"], 0), _dev(h["gs"][2], 1), _dev(h["m"], 2), _dev(h["v"], 3)
    vmax, xbufs = _devx([t * 1.5 for t in h["v"]])
    g[VMAX_ALONE][-1] = float("inf")
    before = [[t.clone() for t in x] for x in (p, m, v, vmax)]
    st = _state(scale=65536.0, tracker=5, adam_step=2, skipped=3)
    _ex_step(p, g, m, v, vmax=vmax, flags=L.OPT_AMSGRAD | L.OPT_DECOUPLED, state=st, max_norm=1.0)
    s = _read(st)
    assert s.found_inf == 1 and s.adam_step == 2 and s.skipped == 4 and s.scale == 32768.0 and s.growth_tracker == 0
    for now, was in zip((p, m, v, vmax), before):
        assert _same(now, was)
    assert _guards_intact(xbufs, XOFF)
    g[VMAX_ALONE][-1] = 0.5                                     # the next, clean step is applied
    _ex_step(p, g, m, v, vmax=vmax, flags=L.OPT_AMSGRAD | L.OPT_DECOUPLED, state=st, max_norm=1.0)
    s = _read(st)
    assert s.found_inf == 0 and s.adam_step == 3 and s.skipped == 4
    # (clipped to norm 1 the new v stays below vmax = 1.5 v everywhere: the maximum keeps its bits, p / m / v move)
    assert not _same(p, before[0]) and not _same(v, before[2]) and _same(vmax, before[3])


# ---------------------------------------------------------------- accumulation
def _accum(acc, g):
    arr = (L.OptAccumTensor * len(acc))()
    for i in range(len(acc)):
        arr[i].acc, arr[i].g, arr[i].n = L.ptr(acc[i]), L.ptr(g[i]), acc[i].numel()
    L.check(L.load().vog_opt_accum_f32(arr, len(acc), L.stream_ptr()), "vog_opt_accum_f32")
    torch.cuda.synchronize()


def test_accum_is_torchs_sum_bit_for_bit_and_deterministic():
    """acc at the offsets of the p column, g at those of the g column: a scalar head with 16-byte accesses behind it (1, 1) and
    no common alignment (1, 2) are both in the set; 79 tensors are three launches."""
    h = _host()
    a_off, g_off = [o[0] for o in OFFSETS], [o[1] for o in OFFSETS]
    runs = []
    for _ in range(2):
        acc, abufs = _devx(h["gs"][0], a_off)
        g, gbufs = _devx(h["gs"][1], g_off)
        _accum(acc, g)
        for i in range(len(acc)):
            assert torch.equal(acc[i].cpu(), h["gs"][0][i] + h["gs"][1][i]), (i, SIZES[i])
            assert torch.equal(g[i].cpu(), h["gs"][1][i]), i
        _accum(acc, _devx(h["gs"][2], g_off)[0])
        for i in range(len(acc)):
            assert torch.equal(acc[i].cpu(), (h["gs"][0][i] + h["gs"][1][i]) + h["gs"][2][i]), (i, SIZES[i])
        assert _guards_intact(abufs, a_off) and _guards_intact(gbufs, g_off)
        runs.append(acc)
    assert _same(runs[0], runs[1])


# ---------------------------------------------------------------- trainer
def _second_batch(dev):
    """Another batch of the same shape: the visual features of `dev`, damped."""
    return {k: (v * 0.5 if k in ("pad_region_feature", "seg_feature_for_frms") else v) for k, v in dev.items()}


def _trainer(built, **kw):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = built
    return trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, **kw)


def test_trainer_accumulates_two_micro_batches_bit_for_bit():
    """accum_steps = 2 on (a, b) against `_optimizer_step` on (ga + gb) * 0.5 formed in torch: one fp32 add, and the factor
    is a power of two - parameters, m and v are bit-equal after two windows."""
    built = _build(NAME)
    a = built[6]
    b = _second_batch(a)
    acc, ref = _trainer(built, accum_steps=2), _trainer(built)
    for w in range(2):
        la, lb = acc.step(a), acc.step(b)
        assert acc.adam_step == w + 1 and acc.num_it == 2 * (w + 1) and acc._acc_n == 0
        (ra, ga), (rb, gb) = ref.gradients(a), ref.gradients(b)
        assert float(la["loss"]) == float(ra["loss"]) and float(lb["loss"]) == float(rb["loss"])
        assert any(not torch.equal(ga[k], gb[k]) for k in ga)
        ref.num_it += 2
        ref._optimizer_step({k: (ga[k] + gb[k]) * 0.5 for k in ga})
    assert ref.adam_step == 2 and set(acc.m) == set(ref.m)
    for k in acc.params:
        assert torch.equal(acc.params[k], ref.params[k]), k
    for k in acc.m:
        assert torch.equal(acc.m[k], ref.m[k]) and torch.equal(acc.v[k], ref.v[k]), k
    # inside a window nothing is applied; gradients() neither reads nor changes it
    before = {k: v.clone() for k, v in acc.params.items()}
    acc.step(a)
    assert acc._acc_n == 1 and acc.adam_step == 2 and acc.num_it == 5
    acc.gradients(b)
    assert acc._acc_n == 1 and all(torch.equal(acc.params[k], before[k]) for k in before)
    acc.step(b)
    assert acc._acc_n == 0 and acc.adam_step == 3 and any(not torch.equal(acc.params[k], before[k]) for k in before)


def test_trainer_accumulates_three_micro_batches_against_float64():
    """accum_steps = 3: the factor 1 / 3 is not exact, so the comparison is with float64 within the one-step bounds (p at
    2^-22 |p| + 1e-4 lr). Those bounds are relative to the AVERAGED gradient and follow from fp32 roundings only where the
    partial sums are no larger than the total, so the window is three calls on one batch (2 g is exact, 3 g one rounding, then
    the product with fl(1 / 3)); windows over different batches are compared bit for bit in the test above."""
    built = _build(NAME)
    a = built[6]
    acc, ref = _trainer(built, accum_steps=3), _trainer(built)
    _, g = ref.gradients(a)
    for k in range(3):
        acc.step(a)
        assert acc.adam_step == (1 if k == 2 else 0) and acc.num_it == k + 1
    lr, b1, b2, eps = (float(np.float32(x)) for x in (1e-4, 0.9, 0.99, 1e-8))
    wm = wv = wp = 0.0
    for k in g:
        g64 = (g[k].double() + g[k].double() + g[k].double()) / 3.0
        m = (1 - b1) * g64
        v = (1 - b2) * g64 * g64
        p = ref.params[k].double() - lr / (1 - b1) * (m / (v.sqrt() / math.sqrt(1 - b2) + eps))
        nz = g64 != 0
        if bool(nz.any()):
            wm = max(wm, float(((acc.m[k].double() - m).abs()[nz] / m.abs()[nz]).max()))
            wv = max(wv, float(((acc.v[k].double() - v).abs()[nz] / v[nz]).max()))
        assert bool((acc.m[k][~nz] == 0).all()) and bool((acc.v[k][~nz] == 0).all())
        wp = max(wp, float(((acc.params[k].double() - p).abs() / (2.0 ** -22 * p.abs() + 1e-4 * lr)).max()))
    print(f"three micro-batches: worst m {wm:.2e}, v {wv:.2e}, p error / bound {wp:.3f}")
    assert wm <= 1e-6 and wv <= 1e-6 and wp <= 1.0, (wm, wv, wp)


def test_flush_applies_a_partial_window_with_its_own_count():
    built = _build(NAME)
    a = built[6]
    acc, one = _trainer(built, accum_steps=3), _trainer(built)
    acc.flush()                                                 # an empty window: nothing happens
    assert acc.adam_step == 0 and not acc.m
    acc.step(a)
    assert acc.adam_step == 0 and acc.num_it == 1
    acc.flush()                                                 # one call of three: that call's gradient, grad_scale = 1
    one.step(a)
    assert acc.adam_step == 1 and acc.num_it == 1 and acc._acc_n == 0
    for k in acc.params:
        assert torch.equal(acc.params[k], one.params[k]), k
    acc.flush()
    assert acc.adam_step == 1 and all(torch.equal(acc.params[k], one.params[k]) for k in acc.params)


# ---------------------------------------------------------------- state interchange with torch.optim
def _two_groups(built):
    keys = [k for k, v in _sd(built[1]).items() if v.is_floating_point()]
    half = len(keys) // 2                   # (torch numbers parameters group by group: with the first half of the state-dict
    return keys, half, [{"params": keys[:half], "weight_decay": 0.01}, {"params": keys[half:]}]      # order in group 0 both agree)


def _torch_twin(tr, keys, osd):
    clones = [torch.nn.Parameter(tr.params[k].detach().cpu().double().clone()) for k in keys]
    opt = torch.optim.AdamW([{"params": [clones[i] for i in g["params"]]} for g in osd["param_groups"]], amsgrad=True, foreach=False)
    opt.load_state_dict(osd)
    for g in opt.param_groups:              # the hyperparameters as the float32 numbers the C ABI takes (1 - float32(0.99) is 9.5e-7 from 0.01)
        g["lr"], g["eps"], g["weight_decay"] = (float(np.float32(g[k])) for k in ("lr", "eps", "weight_decay"))
        g["betas"] = tuple(float(np.float32(b)) for b in g["betas"])
    return clones, opt


def _one_more_step(tr, a, keys, clones, opt, what):
    """One step on both sides from equal states -> compared within the one-step bounds (decoupled: 2^-22 |p|)."""
    _, g = tr.gradients(a)
    lr, b1 = float(np.float32(tr.lr)), float(np.float32(tr.betas[0]))
    terms = {}
    pairs = [(k, q) for k, q in zip(keys, clones) if k in g]    # (parameters the model does not use get no gradient and no state)
    assert len(pairs) >= 40 and set(tr.m) == set(g)
    for k, q in pairs:
        q.grad = g[k].detach().cpu().double()
        terms[k] = (b1 * opt.state[q]["exp_avg"]).abs() + ((1 - b1) * q.grad).abs()
    opt.step()
    tr.step(a)
    wm = wv = wx = wp = 0.0
    for k, q in pairs:
        st = opt.state[q]
        nz = terms[k] != 0
        wm = max(wm, float(((tr.m[k].cpu().double() - st["exp_avg"]).abs()[nz] / terms[k][nz]).max()))
        for mine, ref in ((tr.v[k], st["exp_avg_sq"]), (tr.vmax[k], st["max_exp_avg_sq"])):
            pos = ref > 0
            wv = max(wv, float(((mine.cpu().double() - ref).abs()[pos] / ref[pos]).max()))
            assert bool((mine.cpu()[~pos] == 0).all())
        wp = max(wp, float(((tr.params[k].cpu().double() - q.data).abs() / (2.0 ** -22 * q.data.abs() + 1e-4 * lr)).max()))
    print(f"{what}: worst m {wm:.2e}, v / vmax {wv:.2e}, p error / bound {wp:.3f}")
    assert wm <= 1e-6 and wv <= 1e-6 and wp <= 1.0, (what, wm, wv, wp)


def test_optimizer_state_crosses_to_torch_adamw_and_back():
    built = _build(NAME)
    a = built[6]
    keys, half, groups = _two_groups(built)
    tr = _trainer(built, optimizer="adamw", amsgrad=True, param_groups=groups)
    tr.step(a)
    tr.step(_second_batch(a))
    osd = tr.optimizer_state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} for s in osd["state"].values())
    for gr, wd in zip(osd["param_groups"], (0.01, 0.0)):
        assert gr["amsgrad"] is True and gr["maximize"] is False and gr["decoupled_weight_decay"] is True and gr["weight_decay"] == wd
    clones, opt = _torch_twin(tr, keys, osd)
    assert [g["weight_decay"] for g in opt.param_groups] == [float(np.float32(0.01)), 0.0] and all(g["amsgrad"] for g in opt.param_groups)
    _one_more_step(tr, a, keys, clones, opt, "trainer -> torch.optim.AdamW")
    # and back: torch's state (after its third step) into a fresh trainer over torch's parameters
    back = trn.FP32Trainer(built[0], comm_for(built[4]), {k: q.data.float() for k, q in zip(keys, clones)}, built[7], lr=1e-4,
                           optimizer="adamw", amsgrad=True, param_groups=groups)
    back.load_optimizer_state_dict(opt.state_dict())
    assert back.adam_step == 3 and set(back.vmax) == set(tr.m)
    assert [g["weight_decay"] for g in back._groups] == [float(np.float32(0.01)), 0.0]
    for k, q in zip(keys, clones):                              # the reference continues from the fp32 state the trainer holds
        q.data.copy_(back.params[k].cpu().double())
        if k not in back.m:
            continue
        for nm, mine in (("exp_avg", back.m), ("exp_avg_sq", back.v), ("max_exp_avg_sq", back.vmax)):
            opt.state[q][nm].copy_(mine[k].cpu().double())
    _one_more_step(back, a, keys, clones, opt, "torch.optim.AdamW -> trainer")
    assert back.adam_step == 4
    # plain Adam's own load_state_dict accepts a state without the AdamW key as well
    plain = _trainer(built, amsgrad=True)
    plain.step(a)
    posd = plain.optimizer_state_dict()
    assert "decoupled_weight_decay" not in posd["param_groups"][0] and posd["param_groups"][0]["amsgrad"] is True
    twin = [torch.nn.Parameter(plain.params[k].detach().cpu().double().clone()) for k in keys]
    torch.optim.Adam(twin, amsgrad=True).load_state_dict(posd)


def test_a_state_without_amsgrad_is_refused_by_an_amsgrad_trainer():
    built = _build(NAME)
    plain = _trainer(built)
    plain.step(built[6])
    osd = plain.optimizer_state_dict()
    assert all("max_exp_avg_sq" not in s for s in osd["state"].values())
    with pytest.raises(ValueError, match="max_exp_avg_sq"):
        _trainer(built, amsgrad=True).load_optimizer_state_dict(osd)
    ams = _trainer(built, amsgrad=True)
    ams.step(built[6])
    _trainer(built).load_optimizer_state_dict(ams.optimizer_state_dict())       # the other way round the maximum is dropped


# ---------------------------------------------------------------- Learner
def _learner(tmp_path, uid, n_train, load_opt=False):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    comm = comm_for(c)
    B, ncmp = batch["num_cmp_msk"].shape
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one] * n_train, valid_dl=[one], test_dl=[one])
    cfg.hip.train_accum_steps, cfg.hip.train_plateau_factor, cfg.hip.train_plateau_patience = 2, 0.5, 0
    cfg.train.use_reduce_lr_plateau = True
    cfg.train.load_opt = load_opt
    evl = sel_mod.get_mdl_loss_eval(cfg)["eval"](cfg, comm, torch.device("cuda", 0))
    return tu.Learner(uid=uid, data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)


def _fit(learn, epochs, lr):
    """-> (the learning rate after every epoch, one parameter after every epoch, the validation metrics)."""
    lrs, snaps = [], []
    key = "lin2.0.weight"

    def log(_):
        lrs.append(learn.trainer.lr)
        snaps.append(learn.trainer.params[key].clone())
    hist = learn.fit(epochs=epochs, lr=lr, log=log)
    return lrs, snaps, [h[f"val_{learn.met_keys[0]}"] for h in hist]


def _torch_plateau(lr0, mets, state=None):
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=lr0)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=0)
    if state is not None:
        sched.load_state_dict(state)
    out = []
    for m in mets:
        sched.step(m)
        out.append(opt.param_groups[0]["lr"])
    return out, sched


def test_learner_steps_the_plateau_scheduler_and_applies_the_odd_batch(tmp_path):
    learn = _learner(tmp_path, "V0", 3)
    assert learn.trainer.accum_steps == 2 and learn.trainer.optimizer == "adam"
    lrs, snaps, mets = _fit(learn, 3, 1e-4)
    want, sched = _torch_plateau(1e-4, mets)
    print(f"validation metrics {mets}: lr after each epoch {lrs}, torch's {want}")
    assert lrs == want and learn.lr == want[-1]
    # three batches, windows of two: two updates per epoch (the odd batch through flush), three calls
    assert learn.trainer.num_it == 9 and learn.trainer.adam_step == 6
    learn.save_model_dict()
    ck = torch.load(learn.model_file.open("rb"), weights_only=False)
    assert ck["scheduler_state_dict"] == learn.lr_scheduler.state_dict()
    assert {k: ck["scheduler_state_dict"][k] for k in ("best", "num_bad_epochs", "last_epoch")} == \
           {k: sched.state_dict()[k] for k in ("best", "num_bad_epochs", "last_epoch")}
    # a resumed Learner continues the sequence: its rates are torch's, continued from the saved state
    again = _learner(tmp_path, "V0", 3, load_opt=True)
    assert again.trainer.lr == want[-1] and again.trainer.adam_step == 6 and again.trainer.num_it == 9
    lrs2, _, mets2 = _fit(again, 2, None)
    want2, _ = _torch_plateau(want[-1], mets2, state=sched.state_dict())
    assert lrs2 == want2, (lrs2, want2)
    # the odd batch was applied: a run over the first two batches only ends its first epoch elsewhere
    short = _learner(tmp_path, "V1", 2)
    _, snaps_short, _ = _fit(short, 1, 1e-4)
    assert short.trainer.adam_step == 1 and not torch.equal(snaps[0], snaps_short[0])
