"""Mixed-precision training (the library's "amp" switch): `torch.autocast("cuda")` around the autograd path and
`FP32Trainer(amp=...)` run every product with 16-bit operands and fp32 accumulation, the BiLSTM recurrence in the fused
kernels. Checked against the trainer (autograd = closed loop), against the fp32 step (the bounds of the bf16_gemm test),
operator by operator against torch restatements whose product operands are rounded the same way, over Adam steps
(bf16; f16 with GradScaler), in train mode, for leaks into the fp32 path, and through the Learner."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests.gpu_util import comm_for
from tests.test_gpu_autograd import _build, _close, _grads

pytestmark = pytest.mark.gpu

trn = importlib.import_module("vognet-pytorch_amd.train")
BW = importlib.import_module("vognet-pytorch_amd.backward")
L = importlib.import_module("vognet-pytorch_amd.lib")
synth = importlib.import_module("vognet-pytorch_amd.synth")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")

MODES = {"bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2)}


def _sd(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _switch(name=b"amp"):
    import ctypes
    v = ctypes.c_int32(-1)
    assert L.load().vog_train_get_int(name, ctypes.byref(v)) == 0
    return v.value


def _compare(g32, g16, what):
    """-> (worst deviation / largest entry, smallest cosine, differs) over the gradients of g32."""
    worst, cos_min, differs = 0.0, 1.0, False
    for k in g32:
        a, b = g32[k].double().reshape(-1), g16[k].double().reshape(-1)
        scale = max(float(a.abs().max()), 1e-12)
        e = float((a - b).abs().max()) / scale
        worst = max(worst, e)
        differs |= e > 1e-6
        if float(a.norm()) > 0:
            cos_min = min(cos_min, float(a @ b / (a.norm() * b.norm())))
    print(what, "worst deviation", worst, "min cosine", cos_min)
    return worst, cos_min, differs


# ---------------------------------------------------------------- autograd under autocast = FP32Trainer(amp=...)
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["small/vog_spat", "full/cfg2_vog_spat_gt5_bs4"])
def test_autocast_equals_amp_trainer(name, mode):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    lib = L.load()
    tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp=mode)
    assert lib.vog_train_set_int(b"f32_products", 0) == 0
    ld_tr, ref = tr.gradients(dev)
    assert _switch(b"f32_products") == 0, "an amp step launched fp32 product kernels"
    assert _switch() == 0 and _switch(b"bf16_gemm") == 0
    mdl.eval().requires_grad_(True)
    with torch.autocast("cuda", dtype=MODES[mode][0]):
        out = mdl(dev)
        ld = loss_fn(out, dev)
    assert _switch() == 0
    assert out["mdl_outs"].dtype == torch.float32
    ld["loss"].backward()                                       # outside autocast: the backward keeps the forward's mode
    assert _switch() == 0
    assert abs(float(ld["loss"].detach()) - float(ld_tr["loss"])) <= 1e-6 * abs(float(ld_tr["loss"]))
    got = _grads(mdl)
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert got[k].dtype == torch.float32
        _close(got[k], v.cpu(), 1e-6, k)


# ---------------------------------------------------------------- close to the fp32 step
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_spat_r128", "small/vog_sep_cmpmsk", "small/vog_temp",
                                  "small/vog_spat_3layers", "full/cfg2_vog_spat_gt5_bs4", "full/cfg2_ragged",
                                  "full/cfg5_vog_svsq_gt5_bs16"])
def test_amp_step_close_to_fp32(name, mode):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    t32 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    t16 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp=mode)
    l32, g32 = t32.gradients(dev)
    l16, g16 = t16.gradients(dev)
    assert abs(float(l16["loss"]) - float(l32["loss"])) <= 1e-3 * abs(float(l32["loss"])), (float(l16["loss"]), float(l32["loss"]))
    worst, cos_min, differs = _compare(g32, g16, f"{name} {mode}")
    assert differs and worst <= 0.2 and cos_min >= 0.99, (worst, cos_min)


# ---------------------------------------------------------------- operator level: torch restatements with rounded operands
_ACC = [torch.float32]          # the restatements' product accumulation type (float64: the same math, other last bits)


def _mm(a, b):
    return (a.to(_ACC[0]) @ b.to(_ACC[0])).float()


class _RMM(torch.autograd.Function):
    """r(a) @ r(b) with r = rounding to the 16-bit type; the backward's two products round their operands too."""

    @staticmethod
    def forward(ctx, a, b, dt):
        ra, rb = a.to(dt).float(), b.to(dt).float()
        ctx.save_for_backward(ra, rb)
        ctx.dt = dt
        return _mm(ra, rb)

    @staticmethod
    def backward(ctx, g):
        ra, rb = ctx.saved_tensors
        rg = g.to(ctx.dt).float()
        return _mm(rg, rb.transpose(-1, -2)), _mm(ra.transpose(-1, -2), rg), None


def _check(mode, got, ref, alt, what):
    """got (device) against ref (the restatement), in the largest single deviation and in norm, both relative to ref.
    f16: 1e-3 and 1e-3. bf16: one bf16 unit (2^-8) and 1e-2 - or twice the spread between ref and alt (the same restatement
    accumulating its products in float64) where that is larger: the device sums in another order than either, so now and
    then an activation rounds to the neighbouring bf16 value, and where a tensor is ill-conditioned (sums that cancel) the
    restatements themselves disagree by more than a unit. Measured (profiles/amp_kernel_deviations.txt): every bf16 tensor
    within 3e-3 / 1.2e-3 except the embedding gradient at Bn = 16, R = 1024 (3.1e-2 / 2.5e-2, where ref and alt differ by
    3.1e-2 in the largest entry); f16 within 4e-4 / 1.9e-4. Prints the numbers of every check."""
    got, ref, alt = (t.detach().cpu().double().reshape(ref.shape) for t in (got, ref, alt))
    scale, nrm = max(float(ref.abs().max()), 1e-12), max(float(ref.norm()), 1e-12)
    e_max, e_nrm = float((got - ref).abs().max()) / scale, float((got - ref).norm()) / nrm
    s_max, s_nrm = float((alt - ref).abs().max()) / scale, float((alt - ref).norm()) / nrm
    t_max, t_nrm = (1e-3, 1e-3) if mode == "f16" else (max(2.0 ** -8, 2 * s_max), max(1e-2, 2 * s_nrm))
    print(f"DEV {mode} {what}: max {e_max:.2e} (spread {s_max:.2e}, bound {t_max:.2e}) norm {e_nrm:.2e} "
          f"(spread {s_nrm:.2e}, bound {t_nrm:.2e})")
    assert e_max <= t_max and e_nrm <= t_nrm, (what, e_max, t_max, e_nrm, t_nrm)


def _lin(x, w, b, dt, relu=True):
    y = _RMM.apply(x, w.t(), dt) + b
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("R", [32, 128, 1024])
@pytest.mark.parametrize("Bn", [1, 4, 16, 24])
def test_language_amp_vs_rounded_restatement(Bn, R, mode):
    dt, amp = MODES[mode]
    g = torch.Generator().manual_seed(Bn * 77 + R)
    E, nsrl, V, D, Lo, layers = 32, 3, 11, 48, 40, 2
    lens = [1] + [int(v) for v in torch.randint(1, 9, (Bn - 1,), generator=g)] if Bn > 1 else [1]
    if Bn > 2:
        lens[2] = 9
    T = max(lens)
    sl = T + 2
    sc = 1.0 / math.sqrt(R)
    P = {"emb": torch.randn(V + 1, E, generator=g) * 0.5, "wp": torch.randn(D, 2 * R, generator=g) * sc,
         "bp": torch.randn(D, generator=g) * 0.1, "wa": torch.randn(Lo, 2 * D, generator=g) / math.sqrt(2 * D),
         "ba": torch.randn(Lo, generator=g) * 0.1}
    for l in range(layers):
        K = E if l == 0 else 2 * R
        for dr in range(2):
            P[f"wih{l}{dr}"] = torch.randn(4 * R, K, generator=g) / math.sqrt(K)
            P[f"whh{l}{dr}"] = torch.randn(4 * R, R, generator=g) * sc
            P[f"bih{l}{dr}"] = torch.randn(4 * R, generator=g) * 0.1
            P[f"bhh{l}{dr}"] = torch.randn(4 * R, generator=g) * 0.1
    words = torch.randint(0, V, (Bn, 1, nsrl, sl), generator=g)
    mask = torch.full((Bn, 1, sl), -1, dtype=torch.int64)
    for b, ln in enumerate(lens):
        mask[b, 0, :ln] = torch.randint(0, nsrl * sl, (ln,), generator=g)
    cap = torch.stack([torch.stack([torch.sort(torch.randint(0, ln, (2,), generator=g)).values for _ in range(nsrl)])
                       for ln in lens]).unsqueeze(1)
    d_le = torch.randn(Bn * nsrl, Lo, generator=g)
    d_hid = torch.randn(Bn, D, generator=g)                        # the sep verb head's gradient enters at state slot T

    def restate():                                                  # (packed BiLSTM: a sentence's state is frozen past its length)
        leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        m = mask.reshape(Bn, sl)
        tok = torch.where(m < 0, torch.full_like(m, V), torch.gather(words.reshape(Bn, nsrl * sl), 1, m.clamp(min=0)))[:, :T]
        x = leaves["emb"][tok]                                          # [Bn, T, E]
        ln_t = torch.tensor(lens)
        fin = []
        for l in range(layers):
            outs = []
            for dr in range(2):
                xg = _RMM.apply(x.reshape(Bn * T, -1), leaves[f"wih{l}{dr}"].t(), dt).reshape(Bn, T, 4 * R) + (leaves[f"bih{l}{dr}"] + leaves[f"bhh{l}{dr}"])
                h = torch.zeros(Bn, R)
                c = torch.zeros(Bn, R)
                out = [torch.zeros(Bn, R) for _ in range(T)]
                for s in range(T):
                    act = (s < ln_t)
                    pos = (ln_t - 1 - s).clamp(min=0) if dr else torch.full((Bn,), s)
                    gp = _RMM.apply(h, leaves[f"whh{l}{dr}"].t(), dt) + xg[torch.arange(Bn), pos]
                    i_, f_, g_, o_ = gp.split(R, dim=1)
                    cn = torch.sigmoid(f_) * c + torch.sigmoid(i_) * torch.tanh(g_)
                    hn = torch.sigmoid(o_) * torch.tanh(cn)
                    a1 = act.unsqueeze(1)
                    c = torch.where(a1, cn, c)
                    h = torch.where(a1, hn, h)
                    for b in range(Bn):
                        if act[b]:
                            out[int(pos[b])] = torch.cat([out[int(pos[b])][:b], hn[b:b + 1], out[int(pos[b])][b + 1:]])
                outs.append(torch.stack(out, 1))
                if l == layers - 1:
                    fin.append(h)
            x = torch.cat(outs, -1)
        full = _lin(x.reshape(Bn * T, 2 * R), leaves["wp"], leaves["bp"], dt).reshape(Bn, T, D)
        c2 = cap.reshape(Bn, nsrl, 2)
        st = torch.gather(full, 1, c2[..., 0].unsqueeze(-1).expand(-1, -1, D))
        en = torch.gather(full, 1, c2[..., 1].unsqueeze(-1).expand(-1, -1, D))
        le = _lin(torch.cat([st, en], -1).reshape(Bn * nsrl, 2 * D), leaves["wa"], leaves["ba"], dt)
        hid = _lin(torch.cat(fin, -1), leaves["wp"], leaves["bp"], dt)
        ((le * d_le).sum() + (hid * d_hid).sum()).backward()
        return le.detach(), full.detach(), hid.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}

    le, full, hid, grads = restate()
    _ACC[0] = torch.float64
    try:
        alt = restate()
    finally:
        _ACC[0] = torch.float32
    # device
    sd = {"lstm_encoder.embed_tokens.weight": P["emb"], "lstm_out_feat_proj.0.weight": P["wp"], "lstm_out_feat_proj.0.bias": P["bp"],
          "srl_arg_words_out_enc.0.weight": P["wa"], "srl_arg_words_out_enc.0.bias": P["ba"]}
    names = {"lstm_encoder.embed_tokens.weight": "emb", "lstm_out_feat_proj.0.weight": "wp", "lstm_out_feat_proj.0.bias": "bp",
             "srl_arg_words_out_enc.0.weight": "wa", "srl_arg_words_out_enc.0.bias": "ba"}
    for l in range(layers):
        for dr, sfx in enumerate(("", "_reverse")):
            for k, s_ in (("weight_ih", "wih"), ("weight_hh", "whh"), ("bias_ih", "bih"), ("bias_hh", "bhh")):
                sd[f"lstm_encoder.lstm.{k}_l{l}{sfx}"] = P[f"{s_}{l}{dr}"]
                names[f"lstm_encoder.lstm.{k}_l{l}{sfx}"] = f"{s_}{l}{dr}"
    batch = {"srl_arg_words_ind": words.cuda(), "srl_arg_word_mask": mask.cuda(),
             "srl_arg_word_mask_len": torch.tensor(lens).reshape(Bn, 1).cuda(), "srl_arg_words_capture": cap.cuda()}
    lib = L.load()
    assert lib.vog_train_set_int(b"amp", amp) == 0
    try:
        fwd = BW.language_backward(sd, batch, T, layers)
        r = BW.language_backward(sd, batch, T, layers, d_lang_enc=d_le.cuda(), forward_scratch=fwd["_scratch"], d_hid=d_hid.cuda())
        torch.cuda.synchronize()
    finally:
        lib.vog_train_set_int(b"amp", 0)
    case = f"lang Bn={Bn} R={R}"
    _check(mode, fwd["_lang_enc"], le, alt[0], f"{case} lang_enc")
    _check(mode, fwd["_full"], full, alt[1], f"{case} full")
    _check(mode, fwd["_hid"], hid, alt[2], f"{case} hid")
    for k, short in names.items():
        _check(mode, r[k], grads[short], alt[3][short], f"{case} {k}")


def _attn_rounded(x, wq, wk, wv, boxes, pe_w, pe_b, n_heads, nsrl, dt):
    S, N, d = x.shape
    xf = x.reshape(S * N, d)
    q, k, v = (_RMM.apply(xf, w.t(), dt).reshape(S, N, d) for w in (wq, wk, wv))
    c = -(-d // n_heads)
    outs, off = [], 0
    for h in range(n_heads):
        dh = min(c, d - off)
        lg = _RMM.apply(q[..., off:off + dh], k[..., off:off + dh].transpose(1, 2), dt)
        if boxes is not None:
            diff = boxes.unsqueeze(2) - boxes.unsqueeze(1)
            bh = torch.relu(diff @ pe_w[h] + pe_b[h])
            lg = lg + bh.repeat(1, nsrl, nsrl)
        p = torch.softmax(lg / math.sqrt(d), dim=-1)
        outs.append(_RMM.apply(p, v[..., off:off + dh], dt))
        off += dh
    return torch.cat(outs, -1)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("S,n,nsrl,d,H", [(2, 20, 1, 512, 3), (3, 7, 2, 32, 3)])
def test_attention_amp_vs_rounded_restatement(S, n, nsrl, d, H, mode):
    dt, amp = MODES[mode]
    g = torch.Generator().manual_seed(S * 1000 + n * 10 + d)
    N = n * nsrl
    x = torch.randn(S, N, d, generator=g)
    ws = [torch.randn(d, d, generator=g) / math.sqrt(d) for _ in range(3)]
    props = torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])
    vw, vh, fdiv = 720.0, 405.0, 10.0
    pe_w, pe_b = torch.randn(H, 5, generator=g), torch.randn(H, generator=g) * 0.3
    d_cat = torch.randn(S, N, d, generator=g)
    bx = (props[:, :5] / torch.tensor([vw, vh, vw, vh, fdiv])).reshape(S, n, 5)

    def restate():
        lv = [t.clone().requires_grad_(True) for t in [x] + ws + [pe_w, pe_b]]
        cat = _attn_rounded(lv[0], lv[1], lv[2], lv[3], bx, lv[4], lv[5], H, nsrl, dt)
        (cat * d_cat).sum().backward()
        return cat.detach(), [t.grad for t in lv]

    cat, grads = restate()
    _ACC[0] = torch.float64
    try:
        alt_cat, alt = restate()
    finally:
        _ACC[0] = torch.float32
    w = {"wq": ws[0].cuda(), "wk": ws[1].cuda(), "wv": ws[2].cuda()}
    boxes = BW._Boxes(props.cuda(), vw, vh, fdiv)
    pe = (pe_w.cuda(), pe_b.cuda())
    xd = x.reshape(S * N, d).cuda().contiguous()
    lib = L.load()
    assert lib.vog_train_set_int(b"amp", amp) == 0 and lib.vog_train_set_int(b"f32_products", 0) == 0
    try:
        f = BW._attn_call(w, pe, xd, S, N, n, H, boxes)
        r = BW._attn_call(w, pe, xd, S, N, n, H, boxes, d_cat=d_cat.reshape(S * N, d).cuda().contiguous())
        torch.cuda.synchronize()
        assert _switch(b"f32_products") == 0              # the 171 / 170 and 11 / 10 head products run on the 16-bit instruction
    finally:
        lib.vog_train_set_int(b"amp", 0)
    case = f"attn d={d} H={H}"
    _check(mode, f["cat"], cat, alt_cat, f"{case} cat")
    got = [r["d_x"].reshape(S, N, d), r["g_wq"], r["g_wk"], r["g_wv"], r["g_pe_w"], r["g_pe_b"]]
    for i, k in enumerate(("d_x", "wq", "wk", "wv", "pe_w", "pe_b")):
        _check(mode, got[i], grads[i], alt[i], f"{case} {k}")


# ---------------------------------------------------------------- Adam steps under autocast
def _fresh_model(name):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval().requires_grad_(True)
    return mdl, dev, loss_fn


def test_adam_steps_under_autocast_bf16_track_fp32():
    name = "small/vog_spat"
    m32, dev, loss_fn = _fresh_model(name)
    m16, _, _ = _fresh_model(name)
    o32 = torch.optim.Adam(m32.parameters(), lr=1e-4, betas=(0.9, 0.99))
    o16 = torch.optim.Adam(m16.parameters(), lr=1e-4, betas=(0.9, 0.99))
    a, b = [], []
    for _ in range(3):
        o32.zero_grad()
        l32 = loss_fn(m32(dev), dev)["loss"]
        l32.backward()
        o32.step()
        o16.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            l16 = loss_fn(m16(dev), dev)["loss"]
        l16.backward()
        o16.step()
        a.append(float(l32.detach()))
        b.append(float(l16.detach()))
    print("losses fp32", a, "autocast bf16", b)
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-2 * abs(x), (a, b)
    assert b[-1] < b[0]


def test_adam_steps_under_autocast_f16_with_grad_scaler():
    name = "small/vog_spat"
    m32, dev, loss_fn = _fresh_model(name)
    m16, _, _ = _fresh_model(name)
    o32 = torch.optim.Adam(m32.parameters(), lr=1e-4, betas=(0.9, 0.99))
    o16 = torch.optim.Adam(m16.parameters(), lr=1e-4, betas=(0.9, 0.99))
    # init_scale 2^10: at the default 2^16 the f16 operands of the embedding's gradient overflow on the first step, and the
    # scaler skips it while it calibrates (test_grad_scaler_sees_overflow_and_skips_the_step)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    a, b = [], []
    for _ in range(3):
        o32.zero_grad()
        l32 = loss_fn(m32(dev), dev)["loss"]
        l32.backward()
        o32.step()
        o16.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            l16 = loss_fn(m16(dev), dev)["loss"]
        scaler.scale(l16).backward()
        scaler.unscale_(o16)
        for n, p in m16.named_parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad).all(), n
        scaler.step(o16)
        scaler.update()
        a.append(float(l32.detach()))
        b.append(float(l16.detach()))
    print("losses fp32", a, "autocast f16 + GradScaler", b, "scale", scaler.get_scale())
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-2 * abs(x), (a, b)


def test_grad_scaler_sees_overflow_and_skips_the_step():
    """Scaled gradients pass through the f16 backward unchanged: a scale the f16 operands cannot hold turns into non-finite
    gradients, which the scaler finds - it skips the step and lowers the scale."""
    mdl, dev, loss_fn = _fresh_model("small/vog_spat")
    opt = torch.optim.Adam(mdl.parameters(), lr=1e-4, betas=(0.9, 0.99))
    before = {n: p.detach().clone() for n, p in mdl.named_parameters()}
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = loss_fn(mdl(dev), dev)["loss"]
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    assert any(not torch.isfinite(p.grad).all() for p in mdl.parameters() if p.grad is not None)
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() < 2.0 ** 40
    for n, p in mdl.named_parameters():
        assert torch.equal(p.detach(), before[n]), n


# ---------------------------------------------------------------- train mode
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_amp_train_mode_dropout_close_to_fp32(mode):
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    t32 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, dropout=True, dropout_seed=7)
    t16 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, dropout=True, dropout_seed=7, amp=mode)
    l32, g32 = t32.gradients(dev)
    l16, g16 = t16.gradients(dev)
    e32, _ = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4).gradients(dev)
    assert abs(float(l32["loss"]) - float(e32["loss"])) > 1e-6 * abs(float(e32["loss"]))     # the masks are on
    assert abs(float(l16["loss"]) - float(l32["loss"])) <= 1e-3 * abs(float(l32["loss"]))
    worst, cos_min, differs = _compare(g32, g16, f"train mode {mode}")
    assert differs and worst <= 0.2 and cos_min >= 0.99, (worst, cos_min)


# ---------------------------------------------------------------- no leaks into the fp32 path
def test_amp_leaves_the_fp32_path_bit_identical():
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)

    def fp32_run():
        tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
        ld, g = tr.gradients(dev)
        mdl.zero_grad(set_to_none=True)
        mdl.eval().requires_grad_(True)
        loss_fn(mdl(dev), dev)["loss"].backward()
        torch.cuda.synchronize()
        return float(ld["loss"]), {k: v.clone() for k, v in g.items()}, _grads(mdl)

    before = fp32_run()
    t16 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16")
    for _ in range(2):
        t16.step(dev)
    assert _switch() == 0
    mdl.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = loss_fn(mdl(dev), dev)["loss"]
    loss.backward()
    assert _switch() == 0
    after = fp32_run()
    assert before[0] == after[0]
    for k in before[1]:
        assert torch.equal(before[1][k], after[1][k]), k
    for k in before[2]:
        assert torch.equal(before[2][k], after[2][k]), k
    # a call that raises leaves the switch off behind it
    bad = {k: v for k, v in dev.items() if k != "pad_proposals"}
    with pytest.raises(Exception):
        t16.gradients(bad)
    assert _switch() == 0 and _switch(b"bf16_gemm") == 0


# ---------------------------------------------------------------- Learner
def test_learner_trains_in_bf16_and_its_checkpoint_loads_into_fp32(tmp_path):
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    comm = comm_for(c)
    B, ncmp = batch["num_cmp_msk"].shape
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one, one], valid_dl=[one], test_dl=[one])
    cfg.hip.train_amp = "bf16"
    sel = sel_mod.get_mdl_loss_eval(cfg)
    evl = sel["eval"](cfg, comm, torch.device("cuda", 0))
    learn = tu.Learner(uid="A0", data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)
    assert learn.trainer.amp == "bf16"
    lib = L.load()
    assert lib.vog_train_set_int(b"f32_products", 0) == 0
    hist = learn.fit(epochs=1, lr=1e-4)
    assert len(hist) == 1 and np.isfinite(hist[0]["trn_loss"]) and learn.num_it == 2
    assert _switch() == 0
    learn.save_model_dict()
    cfg2, sd2, _, _, _, mdl2, _, loss2 = _build(name)
    assert cfg2.hip.train_amp == ""
    learn2 = tu.Learner(uid="A0", data=data, mdl=mdl2, loss_fn=loss2, cfg=cfg2, eval_fn=sel_mod.get_mdl_loss_eval(cfg2)["eval"](cfg2, comm, torch.device("cuda", 0)),
                        comm=comm)
    assert learn2.trainer.amp is None
    for k, v in learn.trainer.state_dict().items():
        assert torch.equal(v, learn2.trainer.params[k]), k
    assert learn2.trainer.num_it == 2
