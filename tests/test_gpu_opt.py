"""The fused optimiser step (vog_opt_step_f32, csrc/optim.hip) and what is wired to it: mode A against the per-tensor
vog_adam_f32 loop (bit for bit), mode B - gradient statistics, clipping, loss scale, overflow skip, scale growth - against a
float64 restatement of clip_grad_norm_ + Adam and against torch.amp.GradScaler, `FP32Trainer(loss_scale=, clip_norm=)`, and
the Learner with `cfg.hip.train_loss_scale` / `train_clip_norm` and its checkpoints.

One seeded tensor set throughout (under 1 M elements): sizes that cover heads, tails and chunk boundaries, 70 small tensors
(more than one launch's table holds), a quadruple whose four views start one element into their buffers (4-byte, not 16-byte
aligned: a scalar head, then 16-byte accesses) and one whose four views start at four different offsets (no common alignment:
one element per lane). |g| lies in [1e-3, 1] with random signs: Adam turns rounding noise around zero into a step of +-lr."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

from tests.gpu_util import comm_for
from tests.test_gpu_autograd import _build

pytestmark = pytest.mark.gpu

trn = importlib.import_module("vognet-pytorch_amd.train")
L = importlib.import_module("vognet-pytorch_amd.lib")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")

SIZES = [1, 3, 171, 256, 4097, 65541, 300001] + list(range(1, 71)) + [5002, 4099]
OFFSETS = [(0, 0, 0, 0)] * (len(SIZES) - 2) + [(1, 1, 1, 1), (1, 2, 3, 0)]        # elements into the buffer: p, g, m, v
MIS = len(SIZES) - 2                                                              # "the misaligned tensor"
# the hyperparameters AS THE C ABI TAKES THEM (float): the float64 restatement computes with the numbers the kernels are given -
# 1 - float(0.99) is 9.5e-7 (relative) away from 0.01, which is no error of the kernels
LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.99, 1e-8))
NAME = "small/vog_spat"


def _draw_grads(gen):
    out = []
    for n in SIZES:
        mag = 1e-3 + (1.0 - 1e-3) * torch.rand(n, generator=gen)
        sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
        out.append((mag * sign).float())
    return out


def _adam64(p, g, m, v, step):
    """One torch.optim.Adam step in float64 -> (p, m, v)."""
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    denom = v.sqrt() / math.sqrt(1 - B2 ** step) + EPS
    return p - LR / (1 - B1 ** step) * (m / denom), m, v


_HOST = {}


def _host():
    """The seeded set on the host, made once and never written to: parameters, three gradient sets, and the Adam state after
    two float64 steps on the first two (rounded to fp32: the state a third step starts from)."""
    if not _HOST:
        gen = torch.Generator().manual_seed(1234)
        p0 = [torch.randn(n, generator=gen) for n in SIZES]
        gs = [_draw_grads(gen) for _ in range(3)]
        p, m, v = [], [], []
        for i in range(len(SIZES)):
            pi, mi, vi = p0[i].double(), torch.zeros(SIZES[i], dtype=torch.float64), torch.zeros(SIZES[i], dtype=torch.float64)
            for s in (1, 2):
                pi, mi, vi = _adam64(pi, gs[s - 1][i].double(), mi, vi, s)
            p.append(pi.float()), m.append(mi.float()), v.append(vi.float())
        _HOST.update(p0=p0, gs=gs, p=p, m=m, v=v)
        assert sum(SIZES) < 2 ** 20
    return _HOST


def _dev(host_list, which, offsets=OFFSETS):
    """Device copies at the offsets of OFFSETS (column `which`): views into buffers of n + 4 elements."""
    out = []
    for t, off in zip(host_list, offsets):
        buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device="cuda")
        view = buf[off[which]:off[which] + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * off[which]
        out.append(view)
    return out


def _state(scale=1.0, tracker=0, adam_step=0, skipped=0):
    h = L.OptState(scale=scale, growth_tracker=tracker, adam_step=adam_step, skipped=skipped)
    return torch.frombuffer(bytearray(bytes(h)), dtype=torch.int32).cuda()


def _read(state):
    return L.OptState.from_buffer_copy(state.cpu().numpy().tobytes())


def _opt_step(p, g, m, v, state=None, step=1, max_norm=0.0, growth=(2.0, 0.5, 2000)):
    lib = L.load()
    arr = (L.OptTensor * len(p))()
    for i in range(len(p)):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = L.ptr(p[i]), L.ptr(g[i]), L.ptr(m[i]), L.ptr(v[i]), p[i].numel()
    a = L.OptArgs()
    a.tensors, a.n_tensors = arr, len(p)
    a.lr, a.beta1, a.beta2, a.eps, a.step = LR, B1, B2, EPS, step
    scratch = None
    if state is not None:
        scratch = torch.empty(int(lib.vog_opt_scratch_bytes(len(p), sum(t.numel() for t in p))), dtype=torch.uint8, device="cuda")
        a.state, a.scratch, a.scratch_bytes = L.ptr(state), L.ptr(scratch), scratch.numel()
        a.max_norm = max_norm
        a.growth_factor, a.backoff_factor, a.growth_interval = growth
    L.check(lib.vog_opt_step_f32(C.byref(a), L.stream_ptr()), "vog_opt_step_f32")
    torch.cuda.synchronize()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- mode A
def test_mode_a_is_bit_identical_to_the_per_tensor_loop():
    h = _host()
    lib = L.load()
    p, m, v = _dev(h["p0"], 0), _dev([torch.zeros_like(t) for t in h["p0"]], 2), _dev([torch.zeros_like(t) for t in h["p0"]], 3)
    # the loop's clones: plain aligned tensors (vog_adam_f32 takes any 4-byte alignment; the bits do not depend on it)
    rp, rm, rv = [t.clone() for t in p], [t.clone() for t in m], [t.clone() for t in v]
    for step in (1, 2, 3):
        g = _dev(h["gs"][step - 1], 1)
        _opt_step(p, g, m, v, step=step)
        for i in range(len(rp)):
            gi = g[i].clone()
            L.check(lib.vog_adam_f32(L.ptr(rp[i]), L.ptr(gi), L.ptr(rm[i]), L.ptr(rv[i]), rp[i].numel(), LR, B1, B2, EPS, step,
                                     L.stream_ptr()), "vog_adam_f32")
        torch.cuda.synchronize()
        for i in range(len(rp)):
            assert torch.equal(p[i], rp[i]) and torch.equal(m[i], rm[i]) and torch.equal(v[i], rv[i]), (step, i, SIZES[i])
    assert not _same(p, _dev(h["p0"], 0))


# ---------------------------------------------------------------- mode A on values that a multiplication by 1 must not move
EDGE_SIZES = [4099, 70]                  # a scalar head, the 16-byte body and a tail | one element per lane
EDGE_OFFSETS = [(1, 1, 1, 1), (1, 2, 3, 0)]
TINY = 1.17549435e-38                    # the smallest normal fp32
DENORMALS = [1e-40, 1.4e-45]


def _edge_values(n, gen, shift, denormals=True):
    """fp32 [n]: ordinary values (|x| in [1e-3, 1]) at every other element, between them a cycle through +-0, +-denormals,
    the smallest normals and magnitudes up to 1e18; `shift` moves the cycle, so that the arrays of one tensor do not meet
    value for value."""
    special = [0.0] + (DENORMALS if denormals else []) + [TINY, 2.5 * TINY, 1e-30, 1e6, 1e12, 1e18]
    special = np.array([s * x for x in special for s in (1.0, -1.0)], dtype=np.float64).astype(np.float32)
    x = ((1e-3 + (1.0 - 1e-3) * torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)).numpy()
    idx = np.arange(n)
    at = (idx + shift) % 2 == 0
    x[at] = special[(idx[at] // 2 + 5 * shift) % len(special)]
    return torch.from_numpy(x)


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _opt_step_ex(p, g, m, v, step, grad_scale):
    """vog_opt_step_ex_f32 in mode A with flags = 0: one group over every tensor, at LR, without decay."""
    arr = (L.OptTensor * len(p))()
    for i in range(len(p)):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = L.ptr(p[i]), L.ptr(g[i]), L.ptr(m[i]), L.ptr(v[i]), p[i].numel()
    ex = L.OptExArgs()
    a = ex.groups.base
    a.tensors, a.n_tensors = arr, len(p)
    a.lr, a.beta1, a.beta2, a.eps, a.step = LR, B1, B2, EPS, step
    group = L.OptGroup(first=0, count=len(p), lr=LR, weight_decay=0.0)
    ex.groups.groups, ex.groups.n_groups = C.pointer(group), 1
    ex.flags, ex.grad_scale = 0, grad_scale
    L.check(L.load().vog_opt_step_ex_f32(C.byref(ex), L.stream_ptr()), "vog_opt_step_ex_f32")
    torch.cuda.synchronize()


def test_mode_a_keeps_the_bits_of_zeros_denormals_and_large_values():
    """The plain step multiplies the gradient by a factor of 1 (the one apply kernel's `gscale`): exact only while fp32
    denormals are kept and nothing is contracted away. Gradients, parameters and both moments (v >= 0) hold +-0, +-1e-40,
    +-1.4e-45, the smallest normals and magnitudes up to 1e18 between ordinary values. Two steps of vog_opt_step_f32, and of
    vog_opt_step_ex_f32 with flags = 0, against the per-tensor vog_adam_f32 loop, compared as int32 (a NaN can neither hide
    nor cause a mismatch); then vog_opt_step_ex_f32 with grad_scale = 0.5 on doubled gradients WITHOUT denormals (doubling a
    denormal is exact, halving it back need not be) against the loop on the gradients themselves."""
    lib = L.load()
    gen = torch.Generator().manual_seed(4321)
    for denormals, runs in ((True, (("vog_opt_step_f32", None, 1.0), ("vog_opt_step_ex_f32", 1.0, 1.0))),
                            (False, (("vog_opt_step_ex_f32 on 2 g", 0.5, 2.0),))):
        host = [[_edge_values(n, gen, k, denormals) for n in EDGE_SIZES] for k in range(5)]          # p, m, v, g of step 1 and 2
        host[2] = [t.abs() for t in host[2]]
        tiny = sum(int(((t.abs() > 0) & (t.abs() < TINY)).sum()) for col in host for t in col)
        assert (tiny > 0) == denormals and all(bool((t == 0).any()) and float(t.abs().max()) == float(np.float32(1e18)) for col in host for t in col)
        rp, rm, rv = ([t.cuda() for t in col] for col in host[:3])
        for step in (1, 2):
            for i, g in enumerate(host[2 + step]):
                L.check(lib.vog_adam_f32(L.ptr(rp[i]), L.ptr(g.cuda()), L.ptr(rm[i]), L.ptr(rv[i]), g.numel(), LR, B1, B2, EPS, step,
                                         L.stream_ptr()), "vog_adam_f32")
            torch.cuda.synchronize()
        assert not _bits_equal(rp, [t.cuda() for t in host[0]])
        for what, grad_scale, times in runs:
            p, m, v = (_dev(host[k], w, EDGE_OFFSETS) for k, w in ((0, 0), (1, 2), (2, 3)))
            for step in (1, 2):
                g = _dev([t * times for t in host[2 + step]], 1, EDGE_OFFSETS)
                if grad_scale is None:
                    _opt_step(p, g, m, v, step=step)
                else:
                    _opt_step_ex(p, g, m, v, step, grad_scale)
            assert _bits_equal(p, rp) and _bits_equal(m, rm) and _bits_equal(v, rv), what


# ---------------------------------------------------------------- mode B against float64
def _reference(gs, scale, max_norm, step):
    """clip_grad_norm_ + Adam in float64 on the host from the fp32 state of _host() -> (norm, coef, p, m, v, m_terms)."""
    h = _host()
    g64 = [g.double() / scale for g in gs]
    norm = math.sqrt(sum(float((g * g).sum()) for g in g64))
    clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    p, m, v, terms = [], [], [], []
    for i, g in enumerate(g64):
        gi = g * clip
        pi, mi, vi = _adam64(h["p"][i].double(), gi, h["m"][i].double(), h["v"][i].double(), step)
        p.append(pi), m.append(mi), v.append(vi)
        terms.append((B1 * h["m"][i].double()).abs() + ((1 - B1) * gi).abs())
    return norm, clip / scale, p, m, v, terms


def _check_mode_b(gs_host, scale, max_norm, what):
    """Bounds (the issue's): grad_norm and coef 1e-5 relative (a fixed-order fp32 tree over < 2^20 elements errs by about
    log2(n) 2^-24 = 1.2e-6); v 1e-6 relative per element; m 1e-6 relative to |b1 m| + |(1 - b1) g coef| per element - the
    magnitude of what is added, equal to |m| unless the two terms cancel (they do in some of 380 k entries, and the rounding
    error of a sum does not shrink with the sum); |p - p_ref| <= 2^-23 |p| + 1e-4 lr (half an ulp of p, doubled, plus a
    hundredfold allowance on the ~1e-6 lr fp32 error of the update; 10^4 below one step, so a wrong bias-correction count
    cannot pass)."""
    h = _host()
    p, g, m, v = _dev(h["p"], 0), _dev(gs_host, 1), _dev(h["m"], 2), _dev(h["v"], 3)
    st = _state(scale=scale, tracker=7, adam_step=2)
    _opt_step(p, g, m, v, state=st, max_norm=max_norm)
    s = _read(st)
    norm, coef, rp, rm, rv, terms = _reference(gs_host, scale, max_norm, 3)
    assert s.found_inf == 0 and s.adam_step == 3 and s.skipped == 0 and s.growth_tracker == 8 and s.scale == scale
    e_norm, e_coef = abs(s.grad_norm - norm) / norm, abs(s.coef - coef) / coef
    wm = wv = wp = 0.0
    for i in range(len(p)):
        pm, pv, pp = m[i].cpu().double(), v[i].cpu().double(), p[i].cpu().double()
        wm = max(wm, float(((pm - rm[i]).abs() / terms[i]).max()))
        wv = max(wv, float(((pv - rv[i]).abs() / rv[i]).max()))
        wp = max(wp, float(((pp - rp[i]).abs() / (2.0 ** -23 * rp[i].abs() + 1e-4 * LR)).max()))
    print(f"{what}: grad_norm {s.grad_norm} (ref {norm}) rel {e_norm:.2e}, coef {s.coef} rel {e_coef:.2e}, worst m {wm:.2e}, "
          f"v {wv:.2e}, p error / bound {wp:.3f}")
    assert e_norm <= 1e-5 and e_coef <= 1e-5, (e_norm, e_coef)
    assert wm <= 1e-6 and wv <= 1e-6, (wm, wv)
    assert wp <= 1.0, wp
    return s, p, m, v


@pytest.mark.parametrize("max_norm", [1.0, 1e4])
def test_mode_b_against_float64_clip_and_adam(max_norm):
    h = _host()
    s, *_ = _check_mode_b(h["gs"][2], 1.0, max_norm, f"max_norm {max_norm}")
    clipped = max_norm < s.grad_norm
    assert clipped == (max_norm == 1.0)                         # one case below the norm (~350), one above
    assert (s.coef < 1.0) == clipped


def test_mode_b_carries_the_scale():
    h = _host()
    s0, p0, m0, v0 = _check_mode_b(h["gs"][2], 1.0, 0.0, "unscaled")
    s1, p1, m1, v1 = _check_mode_b([g * 1024.0 for g in h["gs"][2]], 1024.0, 0.0, "scale 1024")
    assert abs(s1.grad_norm - s0.grad_norm) <= 1e-5 * s0.grad_norm              # the UNSCALED norm
    assert abs(s1.coef * 1024.0 - 1.0) <= 1e-5 and s0.coef == 1.0
    for a, b in zip(p0, p1):
        assert bool(((a.double() - b.double()).abs() <= 2.0 ** -23 * a.double().abs() + 1e-4 * LR).all())


# ---------------------------------------------------------------- overflow, growth, determinism
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_overflow_skips_the_step_and_backs_the_scale_off(bad):
    h = _host()
    p, g, m, v = _dev(h["p"], 0), _dev(h["gs"][2], 1), _dev(h["m"], 2), _dev(h["v"], 3)
    g[MIS][-1] = bad                                            # the last element of the misaligned tensor: its scalar tail
    before = [[t.clone() for t in x] for x in (p, m, v)]
    st = _state(scale=65536.0, tracker=5, adam_step=2)
    _opt_step(p, g, m, v, state=st, max_norm=1.0)
    s = _read(st)
    assert s.found_inf == 1 and s.adam_step == 2 and s.skipped == 1 and s.scale == 32768.0 and s.growth_tracker == 0
    assert not math.isfinite(s.grad_norm)
    assert _same(p, before[0]) and _same(m, before[1]) and _same(v, before[2])
    # the next, clean step is applied with the lower scale
    g[MIS][-1] = 0.5
    _opt_step(p, g, m, v, state=st, max_norm=1.0)
    s = _read(st)
    assert s.found_inf == 0 and s.adam_step == 3 and s.skipped == 1 and s.scale == 32768.0 and s.growth_tracker == 1
    assert not _same(p, before[0])


def test_scale_grows_after_clean_steps_and_stays_fixed_without_an_interval():
    h = _host()
    p, g, m, v = _dev(h["p"], 0), _dev(h["gs"][2], 1), _dev(h["m"], 2), _dev(h["v"], 3)
    st = _state(scale=8.0, adam_step=2)
    _opt_step(p, g, m, v, state=st, growth=(2.0, 0.5, 2))
    s = _read(st)
    assert (s.scale, s.growth_tracker, s.adam_step) == (8.0, 1, 3)
    _opt_step(p, g, m, v, state=st, growth=(2.0, 0.5, 2))
    s = _read(st)
    assert (s.scale, s.growth_tracker, s.adam_step) == (16.0, 0, 4)
    # growth_interval = 0: a fixed scale, on clean steps and on overflow; the overflowing step is still skipped
    st = _state(scale=8.0, adam_step=4)
    for k in range(3):
        _opt_step(p, g, m, v, state=st, growth=(2.0, 0.5, 0))
    s = _read(st)
    assert (s.scale, s.adam_step, s.skipped) == (8.0, 7, 0)
    before = [t.clone() for t in p]
    g[0][0] = float("inf")
    _opt_step(p, g, m, v, state=st, growth=(2.0, 0.5, 0))
    s = _read(st)
    assert (s.scale, s.adam_step, s.skipped, s.found_inf) == (8.0, 7, 1, 1)
    assert _same(p, before)


def test_mode_b_is_deterministic():
    h = _host()
    runs = []
    for _ in range(2):
        p, g, m, v = _dev(h["p"], 0), _dev(h["gs"][2], 1), _dev(h["m"], 2), _dev(h["v"], 3)
        st = _state(scale=4.0, adam_step=2)
        _opt_step(p, g, m, v, state=st, max_norm=1.0)
        runs.append((st.cpu(), p, m, v))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in (1, 2, 3):
        assert _same(runs[0][k], runs[1][k])


def test_scale_grad_multiplies_by_the_device_scale():
    lib = L.load()
    st = _state(scale=1024.0)
    for n, off in ((1, 0), (3, 1), (4, 0), (1031, 3), (70001, 2)):
        buf = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
        x = buf[off:off + n]
        ref = torch.randn(n, generator=torch.Generator().manual_seed(n))
        x.copy_(ref)
        L.check(lib.vog_opt_scale_grad_f32(L.ptr(x), n, L.ptr(st), L.stream_ptr()), "vog_opt_scale_grad_f32")
        assert torch.equal(x.cpu(), ref * 1024.0), (n, off)
        assert float(buf[:off].abs().sum()) == 0.0 and float(buf[off + n:].abs().sum()) == 0.0


# ---------------------------------------------------------------- trainer
def _sd(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _switch(name):
    v = C.c_int32(-1)
    assert L.load().vog_train_get_int(name, C.byref(v)) == 0
    return v.value


def test_trainer_f16_with_loss_scale_tracks_fp32():
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    t32 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    t16 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="f16", loss_scale=2.0 ** 10)
    a, b = [], []
    for _ in range(3):
        a.append(float(t32.step(dev)["loss"]))
        b.append(float(t16.step(dev)["loss"]))
    s = t16.scaler_state()
    print("losses fp32", a, "amp f16 with loss scale 2^10", b, s)
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-2 * abs(x), (a, b)
    assert s["skipped"] == 0 and s["adam_step"] == 3 and t16.adam_step == 3 and s["scale"] == 2.0 ** 10
    ld, g = t16.gradients(dev)
    _, g32 = t32.gradients(dev)
    assert set(g) == set(g32) and all(torch.isfinite(x).all() for x in g.values())
    # unscaled: the size of the fp32 gradients, not 2^10 times it
    n16 = math.sqrt(sum(float((x.double() ** 2).sum()) for x in g.values()))
    n32 = math.sqrt(sum(float((x.double() ** 2).sum()) for x in g32.values()))
    assert 0.5 * n32 <= n16 <= 2.0 * n32, (n16, n32)
    assert _switch(b"amp") == 0 and _switch(b"bf16_gemm") == 0


def test_trainer_skips_an_overflowing_step():
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    ref_loss = float(trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="f16").gradients(dev)[0]["loss"])
    tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="f16", loss_scale=2.0 ** 40)
    before = {k: v.clone() for k, v in tr.params.items()}
    loss = float(tr.step(dev)["loss"])
    s = tr.scaler_state()
    assert s["scale"] == 2.0 ** 39 and s["adam_step"] == 0 and tr.adam_step == 0 and s["skipped"] == 1 and s["found_inf"] == 1
    for k, v in tr.params.items():
        assert torch.equal(v, before[k]), k
    assert all(float(t.abs().max()) == 0.0 for t in tr.m.values()) and all(float(t.abs().max()) == 0.0 for t in tr.v.values())
    assert math.isfinite(loss) and abs(loss - ref_loss) <= 1e-6 * abs(ref_loss), (loss, ref_loss)      # unscaled
    assert all(float(st["step"]) == 0.0 for st in tr.optimizer_state_dict()["state"].values())


def test_trainer_takes_the_decisions_of_torchs_grad_scaler():
    """autocast(f16) + torch.amp.GradScaler + torch.optim.Adam on the autograd path against FP32Trainer(amp='f16', loss_scale=):
    the same skip decision at every one of five steps, the same final scale. The initial scale is raised until torch's
    scaler skips at least once (small/vog_spat overflows its f16 operands at 2^16 already)."""
    for exp in (18, 22, 26, 30):
        cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
        mdl.eval().requires_grad_(True)
        opt = torch.optim.Adam(mdl.parameters(), lr=1e-4, betas=(0.9, 0.99))
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** exp, growth_interval=2)
        tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="f16", loss_scale=2.0 ** exp, growth_interval=2)
        skip_t, skip_h, scales_t, scales_h = [], [], [], []
        for _ in range(5):
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16):
                loss = loss_fn(mdl(dev), dev)["loss"]
            scaler.scale(loss).backward()
            was = scaler.get_scale()
            scaler.step(opt)
            scaler.update()
            skip_t.append(scaler.get_scale() < was)
            scales_t.append(scaler.get_scale())
            tr.step(dev)
            s = tr.scaler_state()
            skip_h.append(bool(s["found_inf"]))
            scales_h.append(s["scale"])
        print(f"init 2^{exp}: torch skips {skip_t} scales {scales_t}; trainer skips {skip_h} scales {scales_h}")
        if any(skip_t):
            break
    assert any(skip_t), "no initial scale up to 2^30 made torch's scaler skip a step"
    assert skip_h == skip_t and scales_h == scales_t
    assert tr.adam_step == 5 - sum(skip_t) and tr.scaler_state()["skipped"] == sum(skip_t)


def test_trainer_clips_to_the_norm():
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    probe = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, clip_norm=1e30)
    probe.step(dev)
    s = probe.scaler_state()
    norm = s["grad_norm"]
    assert s["coef"] == 1.0 and s["scale"] == 1.0 and norm > 0 and s["adam_step"] == 1
    _, g = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4).gradients(dev)
    n64 = math.sqrt(sum(float((x.double() ** 2).sum()) for x in g.values()))
    assert abs(norm - n64) <= 1e-5 * n64, (norm, n64)
    tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, clip_norm=0.5 * norm)
    tr.step(dev)
    s = tr.scaler_state()
    assert abs(s["coef"] - 0.5) <= 1e-5 * 0.5 and abs(s["grad_norm"] - norm) <= 1e-5 * norm, s
    # a mode-A step on half the gradients
    lib = L.load()
    keys, sdt = sorted(g), _sd(sd)
    ref = {k: sdt[k].cuda().float().contiguous().clone() for k in keys}
    half = [(g[k] * 0.5).contiguous() for k in keys]
    zm, zv = [torch.zeros_like(ref[k]) for k in keys], [torch.zeros_like(ref[k]) for k in keys]
    arr = (L.OptTensor * len(keys))()
    for i, k in enumerate(keys):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = L.ptr(ref[k]), L.ptr(half[i]), L.ptr(zm[i]), L.ptr(zv[i]), ref[k].numel()
    a = L.OptArgs()
    a.tensors, a.n_tensors = arr, len(keys)
    a.lr, a.beta1, a.beta2, a.eps, a.step = 1e-4, 0.9, 0.99, 1e-8, 1
    L.check(lib.vog_opt_step_f32(C.byref(a), L.stream_ptr()), "vog_opt_step_f32")
    torch.cuda.synchronize()
    worst = 0.0
    for k in keys:
        d = (tr.params[k].double() - ref[k].double()).abs() / (2.0 ** -23 * ref[k].double().abs() + 1e-4 * 1e-4)
        worst = max(worst, float(d.max()))
    print("clipped step against mode A on half the gradients: worst error / bound", worst)
    assert worst <= 1.0


def test_clipping_only_trainer_keeps_scale_one_over_many_steps():
    """Nothing multiplies a clipping-only trainer's gradients by a scale, so GradScaler's schedule must not run for it: with
    growth_interval = 2 the scale is still 1 after four clean steps, and the fifth step's grad_norm and coef are those of
    the true gradients (float64 norm of `gradients()` at the same parameters), not half of them."""
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    probe = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, clip_norm=1e30)
    probe.step(dev)
    clip = 0.5 * probe.scaler_state()["grad_norm"]
    tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, clip_norm=clip, growth_interval=2)
    fixed = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, clip_norm=clip, growth_interval=0)
    for k in range(4):
        tr.step(dev)
        fixed.step(dev)
        s = tr.scaler_state()
        assert s["scale"] == 1.0 and s["found_inf"] == 0 and s["adam_step"] == k + 1, (k, s)
        assert s == fixed.scaler_state(), (k, s)
    plain = trn.FP32Trainer(cfg, comm_for(c), tr.state_dict(), loss_fn, lr=1e-4)
    _, g = plain.gradients(dev)
    n64 = math.sqrt(sum(float((x.double() ** 2).sum()) for x in g.values()))
    tr.step(dev)
    s = tr.scaler_state()
    want = min(1.0, clip / (n64 + 1e-6))
    print(f"clipping only, fifth step: {s}, float64 norm {n64}, coef {want}")
    assert s["scale"] == 1.0 and s["adam_step"] == 5 and s["skipped"] == 0
    assert abs(s["grad_norm"] - n64) <= 1e-5 * n64 and abs(s["coef"] - want) <= 1e-5 * want, (s, n64, want)
    for k, v in tr.params.items():
        assert torch.isfinite(v).all(), k


def test_scale_one_survives_an_overflow_with_the_schedule_off():
    """What a clipping-only trainer passes (scale 1, growth_interval 0): a non-finite step is skipped, the scale stays 1, and
    the next clean step measures and clips exactly as one on a fresh state does."""
    h = _host()
    fresh = _state(scale=1.0, adam_step=2)
    _opt_step(_dev(h["p"], 0), _dev(h["gs"][2], 1), _dev(h["m"], 2), _dev(h["v"], 3), state=fresh, max_norm=1.0, growth=(2.0, 0.5, 0))
    f = _read(fresh)
    p, g, m, v = _dev(h["p"], 0), _dev(h["gs"][2], 1), _dev(h["m"], 2), _dev(h["v"], 3)
    before = [t.clone() for t in p]
    st = _state(scale=1.0, adam_step=2)
    keep = float(g[MIS][-1])
    g[MIS][-1] = float("inf")
    _opt_step(p, g, m, v, state=st, max_norm=1.0, growth=(2.0, 0.5, 0))
    s = _read(st)
    assert (s.scale, s.found_inf, s.skipped, s.adam_step) == (1.0, 1, 1, 2) and _same(p, before)
    g[MIS][-1] = keep
    _opt_step(p, g, m, v, state=st, max_norm=1.0, growth=(2.0, 0.5, 0))
    s = _read(st)
    assert (s.scale, s.found_inf, s.skipped, s.adam_step) == (1.0, 0, 1, 3)
    assert s.grad_norm == f.grad_norm and s.coef == f.coef and f.coef < 1.0


def test_default_trainer_equals_gradients_plus_per_tensor_loop():
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    lib = L.load()
    scaled = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="f16", loss_scale=2.0 ** 10, clip_norm=1.0)
    scaled.step(dev)
    assert _switch(b"amp") == 0 and _switch(b"bf16_gemm") == 0
    fused = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    loop = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    assert fused.scaler_state()["grad_norm"] is None
    for _ in range(3):
        l1 = fused.step(dev)
        l2, grads = loop.gradients(dev)
        loop.num_it += 1
        loop.adam_step += 1
        for k in sorted(grads):
            p = loop.params[k]
            if k not in loop.m:
                loop.m[k], loop.v[k] = torch.zeros_like(p), torch.zeros_like(p)
            gk = grads[k].contiguous()
            L.check(lib.vog_adam_f32(L.ptr(p), L.ptr(gk), L.ptr(loop.m[k]), L.ptr(loop.v[k]), p.numel(), loop.lr, loop.betas[0],
                                     loop.betas[1], loop.eps, loop.adam_step, L.stream_ptr()), "vog_adam_f32")
        assert float(l1["loss"]) == float(l2["loss"])
    assert fused.adam_step == 3 and set(fused.m) == set(loop.m)
    for k in fused.params:
        assert torch.equal(fused.params[k], loop.params[k]), k
    for k in fused.m:
        assert torch.equal(fused.m[k], loop.m[k]) and torch.equal(fused.v[k], loop.v[k]), k


# ---------------------------------------------------------------- Learner
def _learner(tmp_path, uid, **hip):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    comm = comm_for(c)
    B, ncmp = batch["num_cmp_msk"].shape
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one, one], valid_dl=[one], test_dl=[one])
    load_opt = hip.pop("load_opt", False)
    for k, v in hip.items():
        cfg.hip[k] = v
    cfg.train.load_opt = load_opt
    evl = sel_mod.get_mdl_loss_eval(cfg)["eval"](cfg, comm, torch.device("cuda", 0))
    return tu.Learner(uid=uid, data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)


SCALED = dict(train_amp="f16", train_loss_scale="dynamic", train_clip_norm=1.0)


@pytest.mark.parametrize("scale", ["dynamic", "1024"])
def test_learner_trains_f16_with_loss_scale_and_resumes_the_scaler(tmp_path, scale):
    """'dynamic' starts at 2^16, where this case may skip both of its steps (the saved `step` is then 0, which is asserted
    like any other count); '1024' does not overflow (test_trainer_f16_with_loss_scale_tracks_fp32), so both steps apply."""
    hip_keys = dict(train_amp="f16", train_loss_scale=scale, train_clip_norm=1.0)
    learn = _learner(tmp_path, "S0", **hip_keys)
    tr = learn.trainer
    assert tr.amp == "f16" and tr.loss_scale == (2.0 ** 16 if scale == "dynamic" else 1024.0) and tr.clip_norm == 1.0
    hist = learn.fit(epochs=1, lr=1e-4)
    assert len(hist) == 1 and np.isfinite(hist[0]["trn_loss"]) and learn.num_it == 2
    assert _switch(b"amp") == 0
    learn.save_model_dict()
    s = tr.scaler_state()
    print(f"train_loss_scale {scale}: {s}")
    assert s["adam_step"] + s["skipped"] == 2
    if scale == "1024":
        assert s["adam_step"] == 2 and s["scale"] == 1024.0
    ck = torch.load(learn.model_file.open("rb"), weights_only=False)
    ssd = ck["scaler_state_dict"]
    assert set(ssd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    assert ssd["scale"] == s["scale"] and ssd["_growth_tracker"] == s["growth_tracker"] and ssd["growth_interval"] == 2000
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "num_it", "num_epoch", "cfgtxt", "best_met", "scaler_state_dict"}
    saved = ck["optimizer_state_dict"]["state"]                 # m / v exist after any step, applied or skipped
    assert len(saved) == len(tr.m) > 0 and all(float(st["step"]) == s["adam_step"] for st in saved.values())
    learn2 = _learner(tmp_path, "S0", load_opt=True, **hip_keys)
    s2 = learn2.trainer.scaler_state()
    assert (s2["scale"], s2["growth_tracker"], s2["adam_step"]) == (s["scale"], s["growth_tracker"], s["adam_step"])
    assert learn2.trainer.adam_step == s["adam_step"] and learn2.trainer.num_it == 2
    for k, v in tr.state_dict().items():
        assert torch.equal(v, learn2.trainer.params[k]), k


def test_checkpoints_cross_between_scaling_and_plain_learners(tmp_path):
    plain = _learner(tmp_path, "P0")
    assert plain.trainer.loss_scale is None and plain.trainer.clip_norm is None
    plain.save_model_dict()
    assert "scaler_state_dict" not in torch.load(plain.model_file.open("rb"), weights_only=False)
    into_scaled = _learner(tmp_path, "P0", load_opt=True, **SCALED)          # no scaler state in the file: the configured start
    s = into_scaled.trainer.scaler_state()
    assert (s["scale"], s["growth_tracker"], s["adam_step"]) == (2.0 ** 16, 0, 0)
    scaled = _learner(tmp_path, "Q0", train_amp="f16", train_loss_scale="512")
    assert scaled.trainer.scaler_state()["scale"] == 512.0
    scaled.save_model_dict()
    assert torch.load(scaled.model_file.open("rb"), weights_only=False)["scaler_state_dict"]["scale"] == 512.0
    into_plain = _learner(tmp_path, "Q0", load_opt=True)
    assert into_plain.trainer.loss_scale is None and into_plain.trainer.scaler_state()["scale"] == 1.0
    for k, v in scaled.trainer.state_dict().items():
        assert torch.equal(v, into_plain.trainer.params[k]), k
