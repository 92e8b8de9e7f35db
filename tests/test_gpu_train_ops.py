"""Operator tests of the fp32 training path (csrc/train_*.hip), one C-ABI entry at a time, on a guarded scratch.

Reference: the same operation written with plain torch primitives on the CPU in float64 and differentiated by torch autograd
(nn.LSTM on packed sequences for the recurrence); dropout masks from oracle.vog_oracle.drop_mask. Comparison as in
test_gpu_bwd_ops.close: the largest absolute deviation over the reference tensor's largest entry; 2e-5 for activations and the
gradients that are products (weights, inputs), 1e-4 for the gradients that are sums over all rows (biases, LayerNorm gains and
biases, lin2.2.weight, pe_*, every language-side gradient).

Guard band: every call that takes scratch gets `buf[4096 : 4096 + nb]` of one uint8 buffer whose first 4096 and last
max(65536, nb) bytes hold a fixed pattern; nb comes from the entry's own *_scratch_bytes. After the call both bands must still
hold the pattern, so a write past either end of the scratch is a failed assertion (the column sums' partials, CS_CHUNKS rows
of the summed matrix's width, were the two overruns this file was written around: dh > max(d, dhead) in vog_mul_tail_bwd,
D > max(4R, L) in vog_lang_f32). The band is wider than CS_CHUNKS * 4 * (largest width in a case), so that even an unfixed
overrun would stay inside memory the test owns. nb is the exact extent of the entry's layout (no slack behind the last carve),
so any write past the layout reaches the back band; test_misaligned_scratch_base moves the view off the 256-byte boundary."""
import contextlib
import ctypes as C
import importlib
import math

import pytest
import torch

from oracle.vog_oracle import drop_mask

pytestmark = pytest.mark.gpu
bwd = importlib.import_module("vognet-pytorch_amd.backward")
L = bwd.L
TOL, TOL_SUM = 2e-5, 1e-4
CS_CHUNKS = 64                                   # csrc/train_dev.h
FRONT, PATTERN = 4096, 0xA5
F64 = torch.float64


def close(a, b, tol=TOL, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-12)
    err = float((a - b).abs().max()) / scale
    print(f"    {what}: {err:.3e} (bound {tol:.0e})")
    assert err <= tol, (what, err)
    return err


# ---- the guard band ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def guarded(nb, width=0, shift=0):
    """-> a view of nb bytes (`shift` bytes past a 256-byte boundary) between two pattern-filled bands; on exit: synchronize,
    both bands intact. width: the widest matrix the case sums by columns (the back band has to hold CS_CHUNKS rows of it)."""
    nb = int(nb)
    assert nb > 0, nb
    back = max(65536, nb)
    assert back >= CS_CHUNKS * 4 * width, (back, width)
    at = FRONT + shift
    buf = torch.full((at + nb + back,), PATTERN, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    yield buf[at:at + nb]
    torch.cuda.synchronize()
    for name, lo, hi in (("front", 0, at), ("back", at + nb, at + nb + back)):
        bad = (buf[lo:hi] != PATTERN).nonzero()
        assert bad.numel() == 0, f"{name} guard band of a {nb}-byte scratch overwritten: first at byte {int(bad[0])} of the band, {bad.numel()} bytes"


def tail_call(w, attn, x, **kw):
    head = kw.get("head")
    (M, d), dh, dhead = x.shape, w["w1"].shape[0], (head[0]["wl"].shape[0] if head is not None else 0)
    with guarded(L.load().vog_mul_tail_bwd_scratch_bytes(M, d, dh, dhead), max(d, dh, dhead)) as sc:
        return bwd._tail_call(w, attn, x, scratch=sc, **kw)


def attn_call(w, pe, x, S, N, n, H, boxes, shift=0, **kw):
    with guarded(L.load().vog_attn_f32_scratch_bytes(S, N, n, x.shape[1]), 8, shift) as sc:
        return bwd._attn_call(w, pe, x, S, N, n, H, boxes, scratch=sc, **kw)


def linear_call(x, w, b, relu, **kw):
    with guarded(L.load().vog_linear_f32_scratch_bytes(x.shape[0], w.shape[0]), w.shape[0]) as sc:
        return bwd.linear_f32(x, w, b, relu, scratch=sc, **kw)


def score_head_bwd_call(sd, x, dmo, n_vid, nfrm, nppf, nsrl, **kw):
    (M, d), dhead = x.shape, sd["lin2.0.weight"].shape[0]
    with guarded(L.load().vog_score_head_f32_bwd_scratch_bytes(M, d, dhead), max(d, dhead)) as sc:
        return bwd.score_head_backward(sd, x, dmo, n_vid, nfrm, nppf, nsrl, scratch=sc, **kw)


def _lang_nb(sd, batch, T, layers):
    B, nv, nsrl, _ = batch["srl_arg_words_ind"].shape
    E, R = sd["lstm_encoder.embed_tokens.weight"].shape[1], sd["lstm_encoder.lstm.weight_hh_l0"].shape[1]
    D, Lo = sd["lstm_out_feat_proj.0.weight"].shape[0], sd["srl_arg_words_out_enc.0.weight"].shape[0]
    return int(L.load().vog_lang_f32_scratch_bytes(B * nv, T, nsrl, E, R, layers, D, Lo)), max(4 * R, Lo, D)


def language_call(sd, batch, T, layers, shift=0, **kw):
    nb, width = _lang_nb(sd, batch, T, layers)
    with guarded(nb, width, shift) as sc:
        return bwd.language_backward(sd, batch, T, layers, scratch=sc, **kw)


def dev(t):
    return t.detach().to(torch.float32).cuda().contiguous()


# ---- (a) vog_mul_tail_bwd ---------------------------------------------------------------------------------------------
def _ln(t, g, b):
    m = t.mean(-1, keepdim=True)
    v = ((t - m) ** 2).mean(-1, keepdim=True)
    return (t - m) / torch.sqrt(v + 1e-5) * g + b


def _tail_ref(p, attn, x, geo=None, masks=None):
    """(Rel)EncoderLayer tail: Wo, residual + LN, FFN, residual + LN (+ lin2 and the regroup of its scores) -> (y, mdl_outs)."""
    t = attn @ p["wo"].t()
    t = (t * masks[0] if masks else t) + x
    x1 = _ln(t, p["ln1g"], p["ln1b"])
    u = torch.relu(x1 @ p["w1"].t() + p["b1"]) @ p["w2"].t() + p["b2"]
    u = (u * masks[1] if masks else u) + x1
    y = _ln(u, p["ln2g"], p["ln2b"])
    if geo is None:
        return y, None
    n_vid, nfrm, nsrl, nppf = geo
    logit = torch.relu(y @ p["wl"].t() + p["bl"]) @ p["wl2"].reshape(-1) + p["bl2"]
    return y, logit.reshape(n_vid, nfrm, nsrl, nppf).permute(0, 2, 1, 3).reshape(n_vid, nsrl, nfrm * nppf)


def _tail_params(d, dh, dhead, g):
    r = lambda *s: torch.randn(*s, generator=g)
    p = {"wo": r(d, d) / math.sqrt(d), "ln1g": 1 + 0.2 * r(d), "ln1b": 0.1 * r(d), "w1": r(dh, d) / math.sqrt(d), "b1": 0.1 * r(dh),
         "w2": r(d, dh) / math.sqrt(dh), "b2": 0.1 * r(d), "ln2g": 1 + 0.2 * r(d), "ln2b": 0.1 * r(d)}
    if dhead:
        p.update({"wl": r(dhead, d) / math.sqrt(d), "bl": 0.1 * r(dhead) + 0.2, "wl2": r(1, dhead), "bl2": 0.1 * r(1)})
    return p


SUMS = ("ln1g", "ln1b", "b1", "b2", "ln2g", "ln2b", "bl", "wl2", "bl2")       # gradients that are column sums over all rows
TAIL_W, HEAD_W = ("wo", "ln1g", "ln1b", "w1", "b1", "w2", "b2", "ln2g", "ln2b"), ("wl", "bl", "wl2", "bl2")
# (M, d, dh, dhead), (n_vid, nfrm, nsrl, nppf)
S_MODEL, S_DH, S_DHEAD = (60, 32, 16, 24), (60, 32, 96, 24), (60, 32, 40, 80)   # the model's proportions; dh > max(d, dhead); dhead > dh > d
S_ONE, S_ODD, S_LONG = (1, 5, 3, 2), (30, 130, 70, 9), (2048, 16, 8, 8)         # scalar GEMMs; d % 64 != 0; split-K weight gradients
G60A, G60B = (2, 3, 2, 5), (1, 1, 3, 20)
TAIL_CASES = [
    (S_MODEL, G60A, "head"), (S_DH, G60B, "head"), (S_DHEAD, G60A, "head"), (S_ONE, (1, 1, 1, 1), "head"), (S_ODD, (1, 2, 3, 5), "head"),
    (S_LONG, (2, 4, 8, 32), "head"),
    (S_DH, None, "d_y"), (S_ODD, None, "d_y"), (S_LONG, None, "d_y"),
    (S_DH, None, "fwd"), (S_ONE, None, "fwd"),
    (S_DH, G60A, "want_w1b1"), (S_ODD, None, "want_w1b1"),
    (S_DHEAD, G60B, "want_ln2g"), (S_ONE, None, "want_ln2g"),
    (S_DH, G60B, "drop"), (S_ODD, None, "drop"),
]


@pytest.mark.parametrize("shape,geo,mode", TAIL_CASES)
def test_tail(shape, geo, mode):
    M, d, dh, dhead = shape
    if geo is None:
        dhead = 0
    else:
        assert M == geo[0] * geo[1] * geo[2] * geo[3]
    g = torch.Generator().manual_seed(M * 7 + d * 3 + dh)
    p = _tail_params(d, dh, dhead, g)
    attn, x = torch.randn(M, d, generator=g), torch.randn(M, d, generator=g)
    seed, site = 1234, 210
    masks = [drop_mask(seed, site + 1, (M, d), 0.3).double(), drop_mask(seed, site + 2, (M, d), 0.3).double()] if mode == "drop" else None
    lv = {k: v.to(F64).requires_grad_(True) for k, v in {**p, "attn": attn, "x": x}.items()}
    y, outs = _tail_ref(lv, lv["attn"], lv["x"], geo, masks)
    w = {k: dev(v) for k, v in p.items()}
    kw = {"drop": (0.3, seed, site)} if mode == "drop" else {}
    if mode == "fwd":
        r = tail_call(w, dev(attn), dev(x))
        assert set(r) == {"y", "_keepalive"}
        close(r["y"], y, what="y")
        return
    if geo is not None:
        dmo = torch.randn(outs.shape, generator=g)
        (outs * dmo.double()).sum().backward()
        n_vid, nfrm, nsrl, nppf = geo
        kw["head"] = ({k: w[k] for k in HEAD_W}, dev(dmo), n_vid, nfrm, nppf, nsrl)
    else:
        d_y = torch.randn(M, d, generator=g)
        (y * d_y.double()).sum().backward()
        kw["d_y"] = dev(d_y)
    want, want_dx, want_dattn = None, True, True
    if mode == "want_w1b1":
        want = {"w1", "b1"}
    elif mode == "want_ln2g":
        want, want_dx, want_dattn = {"ln2g"}, False, False
    r = tail_call(w, dev(attn), dev(x), want_y=True, want=want, want_dx=want_dx, want_dattn=want_dattn, **kw)
    close(r["y"], y, what="y")
    if mode == "drop":                                           # the masks were on
        ev = tail_call(w, dev(attn), dev(x))
        assert not torch.allclose(ev["y"], r["y"], atol=1e-3)
    keys = [k for k in TAIL_W + (HEAD_W if geo is not None else ()) if want is None or k in want]
    assert {k for k in r if k.startswith("g_")} == {"g_" + k for k in keys}
    assert ("d_x" in r) == want_dx and ("d_attn" in r) == want_dattn
    for k in keys:
        close(r["g_" + k], lv[k].grad, tol=TOL_SUM if k in SUMS else TOL, what="g_" + k)
    if want_dx:
        close(r["d_x"], lv["x"].grad, what="d_x")
    if want_dattn:
        close(r["d_attn"], lv["attn"].grad, what="d_attn")


# ---- (b) vog_attn_f32 -------------------------------------------------------------------------------------------------
def _attn_ref(x, wq, wk, wv, boxes, pe_w, pe_b, H, nsrl, mask=None):
    S, N, d = x.shape
    q, k, v = x @ wq.t(), x @ wk.t(), x @ wv.t()
    c = -(-d // H)
    outs, off = [], 0
    for h in range(H):
        dh = min(c, d - off)
        lg = q[..., off:off + dh] @ k[..., off:off + dh].transpose(1, 2)
        if boxes is not None:
            diff = boxes.unsqueeze(2) - boxes.unsqueeze(1)
            lg = lg + torch.relu(diff @ pe_w[h] + pe_b[h]).repeat(1, nsrl, nsrl)
        pr = torch.softmax(lg / math.sqrt(d), dim=-1)
        if mask is not None:
            pr = pr * mask[:, h]                                   # element ((s * H + h) * N + i) * N + j
        outs.append(pr @ v[..., off:off + dh])
        off += dh
    return torch.cat(outs, -1)


G_TAIL70 = (2, 35, 2, 24, 5)                     # N = 70 > 64, N % 64 != 0 (the row kernels' lane loop); heads of 5/5/5/5/4
ATTN_CASES = [
    ((2, 5, 3, 48, 3), True, "drop"), (G_TAIL70, True, "drop"),
    (G_TAIL70, True, "plain"), (G_TAIL70, False, "plain"),
    (G_TAIL70, True, "accumulate"), ((3, 7, 1, 32, 3), False, "accumulate"),
    ((2, 5, 3, 48, 3), True, "want_wk"), (G_TAIL70, False, "want_wk"),
    ((2, 5, 3, 48, 3), True, "want_pe"), (G_TAIL70, True, "want_pe_nodx"),
    ((3, 6, 1, 8, 8), True, "plain"), ((2, 4, 2, 5, 5), False, "plain"),          # H == d: one feature per head
]


@pytest.mark.parametrize("geo,rel,mode", ATTN_CASES)
def test_attention(geo, rel, mode):
    S, n, nsrl, d, H = geo
    N = n * nsrl
    g = torch.Generator().manual_seed(S * 1000 + n * 10 + d)
    x = torch.randn(S, N, d, generator=g)
    ws = [torch.randn(d, d, generator=g) / math.sqrt(d) for _ in range(3)]
    props = torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])
    vw, vh, fdiv = 720.0, 405.0, 10.0
    pe_w, pe_b = torch.randn(H, 5, generator=g), torch.randn(H, generator=g) * 0.3
    d_cat = torch.randn(S, N, d, generator=g)
    prefill = torch.randn(S * N, d, generator=g)
    lv = [t.to(F64).requires_grad_(True) for t in [x] + ws + [pe_w, pe_b]]
    bx = (props[:, :5].double() / torch.tensor([vw, vh, vw, vh, fdiv], dtype=F64)).reshape(S, n, 5) if rel else None
    seed, site, p = 77, 120, 0.25
    mask = drop_mask(seed, site, (S, H, N, N), p).double() if mode == "drop" else None
    cat = _attn_ref(lv[0], lv[1], lv[2], lv[3], bx, lv[4], lv[5], H, nsrl, mask)
    (cat * d_cat.double()).sum().backward()
    w = {"wq": dev(ws[0]), "wk": dev(ws[1]), "wv": dev(ws[2])}
    boxes = bwd._Boxes(dev(props), vw, vh, fdiv) if rel else None
    pe = (dev(pe_w), dev(pe_b)) if rel else None
    xd, dcd = dev(x.reshape(S * N, d)), dev(d_cat.reshape(S * N, d))
    kw = {"drop": (p, seed, site)} if mode == "drop" else {}
    f = attn_call(w, pe, xd, S, N, n, H, boxes, **kw)
    close(f["cat"], cat.reshape(S * N, d), what="cat")
    if mode == "drop":
        ev = attn_call(w, pe, xd, S, N, n, H, boxes)
        assert not torch.allclose(ev["cat"], f["cat"], atol=1e-3)
    want = {"want_wk": {"wk"}, "want_pe": {"pe"}, "want_pe_nodx": {"pe"}}.get(mode)
    want_dx = mode not in ("want_wk", "want_pe_nodx")
    if mode == "accumulate":
        kw.update(d_x=dev(prefill), accumulate_dx=True)
    r = attn_call(w, pe, xd, S, N, n, H, boxes, d_cat=dcd, want=want, want_dx=want_dx, **kw)
    keys = [k for k in ("wq", "wk", "wv") if want is None or k in want]
    has_pe = rel and (want is None or "pe" in want)
    assert {k for k in r if k.startswith("g_")} == {"g_" + k for k in keys} | ({"g_pe_w", "g_pe_b"} if has_pe else set())
    assert ("d_x" in r) == want_dx
    if want_dx:
        dx = lv[0].grad.reshape(S * N, d)
        close(r["d_x"], dx + prefill.double() if mode == "accumulate" else dx, what="d_x")
    for k in keys:
        close(r["g_" + k], lv[1 + ("wq", "wk", "wv").index(k)].grad, what="g_" + k)
    if has_pe:
        close(r["g_pe_w"], lv[4].grad, tol=TOL_SUM, what="pe_w")
        close(r["g_pe_b"], lv[5].grad, tol=TOL_SUM, what="pe_b")


# ---- (c) vog_linear_f32 -----------------------------------------------------------------------------------------------
# The three products of vog_linear_f32(M, N, K) and the branch of gemm_f32_b each takes (dims of the product as [M', N', K']):
#   y   = x W^T       [M, N, K]  A row-major (ak = 1), B = W with bk = 1:   the only one that can be the weight-stream ("skinny")
#                                kernel: M <= 16, N >= 256, K % 4 == 0 (wide form: N >= 2048)
#   g_w = dpre^T x    [N, K, M]  A column-major (ak = N): never skinny; split-K when M >= 1024 and ceil(K/64) ceil(N/128) <= 96
#   d_x = dpre W      [M, K, N]  B row-major (bk = K): never skinny; split-K when N >= 1024 and ceil(K/64) ceil(M/128) <= 96
# vector tiles need M, N, K all multiples of 4 (and 16-byte aligned operands), anything else is the scalar tile. Split-K cuts K'
# into chunks that are multiples of 16, so its batch strides sa / sb are always multiples of 4: the `scalar` switch behind a
# reduced kchunk cannot fire, and split-K is vector or scalar exactly as the un-split product would be.
LIN_CASES = [
    # M, N, K, rep, relu, options                  y / g_w / d_x
    (64, 32, 48, 1, True, {}),                     # vector tile / vector tile / vector tile
    (33, 7, 9, 1, True, {"acc"}),                  # scalar tile (odd strides) all three; d_x accumulates
    (20, 24, 36, 5, True, {"no_w"}),               # vector tiles, replicated rows; g_w skipped
    (8, 1024, 12, 1, False, {"acc"}),              # skinny <8, 1> / vector tile / vector split-K (K' = 1024: 4 chunks of 256), accumulating
    (3, 1030, 5, 1, True, {"no_b"}),               # scalar tile / scalar tile / scalar split-K (K' = 1030: chunks of 272, last 214)
    (2048, 8, 12, 1, True, {"nobias"}),            # vector tile / vector split-K (K' = 2048: 8 chunks of 256) / vector tile; b = None
    (1500, 7, 5, 2, True, {"acc"}),                # scalar tile / scalar split-K (K' = 1500: chunks of 304, last 284) / scalar tile
    (5, 260, 12, 1, True, {}),                     # skinny <8, 1>, N no multiple of 16 / scalar tile (M % 4 != 0) / scalar tile
    (12, 2050, 8, 1, False, {"no_w", "no_b"}),     # skinny <16, 2> wide, N % 8 != 0 / - / scalar split-K (K' = 2050: chunks of 272, last 146)
    (4, 2048, 16, 1, True, {}),                    # skinny <4, 4> wide / vector tile / vector split-K (K' = 2048)
    (16, 256, 20, 1, True, {"no_dx"}),             # skinny <16, 1> at both thresholds (M = 16, N = 256) / vector tile / -
    (17, 256, 20, 1, True, {}),                    # M = 17: one past the skinny threshold -> scalar tile (M % 4 != 0)
]


@pytest.mark.parametrize("M,N,K,rep,relu,opts", LIN_CASES)
def test_linear(M, N, K, rep, relu, opts):
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b = None if "nobias" in opts else torch.randn(N, generator=g) * 0.1
    col0, wide = 3, N + 6
    dy = torch.randn(M * rep, wide, generator=g)                    # the layer's output gradient sits inside a wider matrix
    prefill = torch.randn(M, K, generator=g)
    xr, wr = x.to(F64).requires_grad_(True), w.to(F64).requires_grad_(True)
    br = b.to(F64).requires_grad_(True) if b is not None else None
    y = xr @ wr.t() + (br if br is not None else 0)
    y = torch.relu(y) if relu else y
    (y.unsqueeze(1).expand(M, rep, N).reshape(M * rep, N) * dy[:, col0:col0 + N].double()).sum().backward()
    r = linear_call(dev(x), dev(w), dev(b) if b is not None else None, relu, dy=dev(dy), dy_col0=col0, rep=rep, want_y=True,
                    want_dx="no_dx" not in opts, d_x=dev(prefill) if "acc" in opts else None, want_w="no_w" not in opts,
                    want_b="no_b" not in opts)
    assert ("g_w" in r) == ("no_w" not in opts) and ("g_b" in r) == (b is not None and "no_b" not in opts)
    assert ("d_x" in r) == ("no_dx" not in opts)
    close(r["y"], y, what="y")
    if "g_w" in r:
        close(r["g_w"], wr.grad, what="g_w")
    if "g_b" in r:
        close(r["g_b"], br.grad, tol=TOL_SUM, what="g_b")
    if "d_x" in r:
        close(r["d_x"], xr.grad + prefill.double() if "acc" in opts else xr.grad, what="d_x")
    f = linear_call(dev(x), dev(w), dev(b) if b is not None else None, relu)           # forward only
    assert set(f) == {"y", "_keepalive"}
    close(f["y"], y, what="y (forward only)")


# The weight-stream rows of LIN_CASES under "amp" = 1 | 2 (both operands rounded to bf16 | f16 behind their loads; one kernel
# template with the fp32 form): the trainer reaches these instances only at model shapes. Forward y only. Reference:
# relu?(x16 @ w16^T + b) in float64 with the operands rounded as tests/test_gpu_amp.py rounds them. A product of two 16-bit values
# is exact in fp32 and at most K = 20 fp32 additions follow, so the restatement's own noise is orders below TOL.
LIN_SKINNY = [c for c in LIN_CASES if c[:3] in {(8, 1024, 12), (12, 2050, 8), (4, 2048, 16), (16, 256, 20)}]


@pytest.mark.parametrize("amp,dt", [(1, torch.bfloat16), (2, torch.float16)], ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K,rep,relu,opts", LIN_SKINNY)
def test_linear_skinny_amp(M, N, K, rep, relu, opts, amp, dt):
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    y = x.to(dt).to(F64) @ w.to(dt).to(F64).t() + b.to(F64)
    y = torch.relu(y) if relu else y
    lib, n32 = L.load(), C.c_int32(-1)
    assert lib.vog_train_set_int(b"amp", amp) == 0 and lib.vog_train_set_int(b"f32_products", 0) == 0
    try:
        f = linear_call(dev(x), dev(w), dev(b), relu)
        assert lib.vog_train_get_int(b"f32_products", C.byref(n32)) == 0 and n32.value == 0
    finally:
        lib.vog_train_set_int(b"amp", 0)
    close(f["y"], y, what=f"y (amp = {amp})")


# ---- (d) vog_lang_f32 -------------------------------------------------------------------------------------------------
NSRL, VOCAB = 3, 11


def _lang_case(Bn, lens, E, R, layers, D, Lo):
    g = torch.Generator().manual_seed(Bn * 77 + E + R + 5 * D + Lo)
    r = lambda *s: torch.randn(*s, generator=g) * 0.3
    T = max(lens)
    sl = T + 2
    P = {"lstm_encoder.embed_tokens.weight": r(VOCAB + 1, E), "lstm_out_feat_proj.0.weight": r(D, 2 * R), "lstm_out_feat_proj.0.bias": r(D),
         "srl_arg_words_out_enc.0.weight": r(Lo, 2 * D), "srl_arg_words_out_enc.0.bias": r(Lo)}
    for l in range(layers):
        for sfx in ("", "_reverse"):
            K = E if l == 0 else 2 * R
            for k, shp in (("weight_ih", (4 * R, K)), ("weight_hh", (4 * R, R)), ("bias_ih", (4 * R,)), ("bias_hh", (4 * R,))):
                P[f"lstm_encoder.lstm.{k}_l{l}{sfx}"] = r(*shp)
    words = torch.randint(0, VOCAB, (Bn, 1, NSRL, sl), generator=g)
    mask = torch.full((Bn, 1, sl), -1, dtype=torch.int64)
    for b, ln in enumerate(lens):
        mask[b, 0, :ln] = torch.randint(0, NSRL * sl, (ln,), generator=g)
    cap = torch.stack([torch.stack([torch.sort(torch.randint(0, ln, (2,), generator=g)).values for _ in range(NSRL)]) for ln in lens]).unsqueeze(1)
    return {"P": P, "words": words, "mask": mask, "cap": cap, "lens": lens, "T": T, "dims": (Bn, E, R, layers, D, Lo),
            "d_le": torch.randn(Bn * NSRL, Lo, generator=g), "d_hid": torch.randn(Bn, D, generator=g)}


def _lang_ref(c, drop=None, with_hid=True, dt=F64):
    """Embedding -> packed BiLSTM layers (one nn.LSTM each, so that the masks between them can be restated) -> Linear + ReLU ->
    start / end gather -> Linear + ReLU; hid = the same projection of [forward state after step len - 1 | reverse state after
    position 0] of the top layer. -> (lang_enc, full, hid, {parameter name: gradient})."""
    Bn, E, R, layers, D, Lo = c["dims"]
    T, lens = c["T"], c["lens"]
    lv = {k: v.to(dt).requires_grad_(True) for k, v in c["P"].items()}
    wflat, m = c["words"].reshape(Bn, -1), c["mask"].reshape(Bn, -1)
    tok = torch.where(m < 0, torch.full_like(m, VOCAB), torch.gather(wflat, 1, m.clamp(min=0)))[:, :T]
    x = lv["lstm_encoder.embed_tokens.weight"][tok]
    if drop:
        x = x * drop_mask(drop[2], 1, (Bn * T, E), drop[0]).to(dt).reshape(Bn, T, E)
    mods = []
    for l in range(layers):
        lstm = torch.nn.LSTM(E if l == 0 else 2 * R, R, num_layers=1, bidirectional=True, batch_first=True).to(dt)
        with torch.no_grad():
            for n_, p_ in lstm.named_parameters():
                p_.copy_(c["P"]["lstm_encoder.lstm." + n_.replace("_l0", f"_l{l}")])
        mods.append(lstm)
        pk = torch.nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False)
        out, (hn, _) = lstm(pk)
        x, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
        if drop:
            x = x * drop_mask(drop[2], 2 + l if l < layers - 1 else 10, (Bn * T, 2 * R), drop[1]).to(dt).reshape(Bn, T, 2 * R)
    wp, bp = lv["lstm_out_feat_proj.0.weight"], lv["lstm_out_feat_proj.0.bias"]
    full = torch.relu(x @ wp.t() + bp)
    hid = torch.relu(torch.cat([hn[0], hn[1]], -1) @ wp.t() + bp)
    c2 = c["cap"].reshape(Bn, NSRL, 2)
    st = torch.gather(full, 1, c2[..., 0].unsqueeze(-1).expand(-1, -1, D))
    en = torch.gather(full, 1, c2[..., 1].unsqueeze(-1).expand(-1, -1, D))
    le = torch.relu(torch.cat([st, en], -1) @ lv["srl_arg_words_out_enc.0.weight"].t() + lv["srl_arg_words_out_enc.0.bias"]).reshape(Bn * NSRL, Lo)
    loss = (le * c["d_le"].to(dt)).sum()
    if with_hid:
        loss = loss + (hid * c["d_hid"].to(dt)).sum()
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items() if ".lstm." not in k}
    for l, lstm in enumerate(mods):
        for n_, p_ in lstm.named_parameters():
            grads["lstm_encoder.lstm." + n_.replace("_l0", f"_l{l}")] = p_.grad
    return le, full.reshape(Bn * T, D), hid, grads


def _lang_dev(c):
    Bn = c["dims"][0]
    batch = {"srl_arg_words_ind": c["words"].cuda(), "srl_arg_word_mask": c["mask"].cuda(),
             "srl_arg_word_mask_len": torch.tensor(c["lens"]).reshape(Bn, 1).cuda(), "srl_arg_words_capture": c["cap"].cuda()}
    return {k: v.cuda() for k, v in c["P"].items()}, batch


LANG_OVER = (3, [5, 2, 7], 8, 4, 2, 40, 5)       # D > max(4R, L): the partials of b_proj used to run into dpre2
LANG_L = (3, [5, 2, 7], 8, 2, 2, 6, 24)          # L > 4R
LANG_4 = (2, [4, 6], 6, 4, 4, 6, 5)              # layers = 4
LANG_WIDE = (4, [1, 9, 4, 9], 16, 12, 2, 70, 5)  # D > 64: more than one column block of partials past 4R = 48
_LANG_CACHE = {}


def _lang(key, drop=None):
    k = (key[0], tuple(key[1])) + key[2:] + (drop,)
    if k not in _LANG_CACHE:                               # one reference per case, shared by the tests below (read-only)
        c = _lang_case(*key)
        _LANG_CACHE[k] = (c, _lang_ref(c, drop=drop))
    return _LANG_CACHE[k]


@pytest.mark.parametrize("key,drop", [(LANG_OVER, None), (LANG_L, None), (LANG_4, None), (LANG_WIDE, None), (LANG_OVER, (0.2, 0.3, 9)),
                                      (LANG_4, (0.2, 0.3, 4))])
def test_language(key, drop):
    c, (le, full, hid, grads) = _lang(key, drop)
    sd, batch = _lang_dev(c)
    r = language_call(sd, batch, c["T"], c["dims"][3], d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda(), drop=drop)
    close(r["_lang_enc"], le, what="lang_enc"); close(r["_full"], full, what="full"); close(r["_hid"], hid, what="hid")
    for k in sd:
        close(r[k], grads[k], tol=TOL_SUM, what=k)
    if drop:
        ev = language_call(sd, batch, c["T"], c["dims"][3])
        assert not torch.allclose(ev["_full"], r["_full"], atol=1e-3)


@pytest.mark.parametrize("need", [("lstm_encoder.lstm.weight_hh_l1_reverse",), ("lstm_encoder.embed_tokens.weight",),
                                  ("srl_arg_words_out_enc.0.bias",)])
def test_language_need_subsets(need):
    """Only the wanted gradients come back (the chain stops above layer 0 / runs to the embedding / returns behind b_arg)."""
    c, (le, full, hid, grads) = _lang(LANG_OVER)
    sd, batch = _lang_dev(c)
    r = language_call(sd, batch, c["T"], c["dims"][3], d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda(), need=set(need))
    assert {k for k in r if not k.startswith("_")} == set(need)
    close(r["_lang_enc"], le, what="lang_enc")
    for k in need:
        close(r[k], grads[k], tol=TOL_SUM, what=k)


@pytest.mark.parametrize("drop", [None, (0.2, 0.3, 9)])
def test_language_forward_scratch_reuse_is_bit_identical(drop):
    c = _lang_case(*LANG_OVER)
    sd, batch = _lang_dev(c)
    T, layers = c["T"], c["dims"][3]
    kw = dict(d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda(), drop=drop)
    a = language_call(sd, batch, T, layers, **kw)
    nb, width = _lang_nb(sd, batch, T, layers)
    with guarded(nb, width) as sc:
        f = bwd.language_backward(sd, batch, T, layers, drop=drop, scratch=sc)
        b = bwd.language_backward(sd, batch, T, layers, forward_scratch=f["_scratch"], **kw)
    for k in sd:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["_lang_enc"], f["_lang_enc"]) and torch.equal(a["_hid"], f["_hid"])


@pytest.mark.parametrize("amp", [1, 2])
@pytest.mark.parametrize("key", [LANG_OVER, LANG_4])
def test_language_guard_band_under_amp(key, amp):
    """The amp layout shares `part` and adds carves of its own: bands and finiteness only (its numerics: test_gpu_amp.py)."""
    c = _lang_case(*key)
    sd, batch = _lang_dev(c)
    lib = L.load()
    assert lib.vog_train_set_int(b"amp", amp) == 0
    try:
        r = language_call(sd, batch, c["T"], c["dims"][3], d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda(), drop=(0.2, 0.3, 9))
    finally:
        lib.vog_train_set_int(b"amp", 0)
    for k in list(sd) + ["_lang_enc", "_full", "_hid"]:
        assert torch.isfinite(r[k]).all(), k


# ---- (d') a scratch that does not start on a 256-byte boundary -----------------------------------------------------------
def _attn_runs(shift):
    S, N, n, d, H = 2, 6, 3, 8, 2
    g = torch.Generator().manual_seed(5)
    x, d_cat = dev(torch.randn(S * N, d, generator=g)), dev(torch.randn(S * N, d, generator=g))
    w = {k: dev(torch.randn(d, d, generator=g) / math.sqrt(d)) for k in ("wq", "wk", "wv")}
    props = torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])
    pe, boxes = (dev(torch.randn(H, 5, generator=g)), dev(torch.randn(H, generator=g) * 0.3)), bwd._Boxes(dev(props), 720.0, 405.0, 10.0)
    f = attn_call(w, pe, x, S, N, n, H, boxes, shift=shift)
    r = attn_call(w, pe, x, S, N, n, H, boxes, shift=shift, d_cat=d_cat)
    assert {"g_wq", "g_wk", "g_wv", "g_pe_w", "g_pe_b", "d_x"} <= set(r)
    return {"cat": f["cat"], **r}


def _lang_runs(shift, layers=1, amp=0):
    c = _lang_case(1, [2], 4, 4, layers, 6, 5)
    sd, batch = _lang_dev(c)
    lib = L.load()
    assert lib.vog_train_set_int(b"amp", amp) == 0
    try:
        f = language_call(sd, batch, c["T"], layers, shift=shift)
        r = language_call(sd, batch, c["T"], layers, shift=shift, d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda())
    finally:
        lib.vog_train_set_int(b"amp", 0)
    assert set(sd) <= set(r)
    return {**{"fwd" + k: f[k] for k in ("_lang_enc", "_full", "_hid")}, **r}


@pytest.mark.parametrize("shift", [1, 252])
@pytest.mark.parametrize("run", [_attn_runs, _lang_runs, lambda s: _lang_runs(s, layers=4, amp=1)], ids=["attn", "lang", "lang_4_layers_bf16"])
def test_misaligned_scratch_base(run, shift):
    """vog_attn_f32 and vog_lang_f32 start their carve at the next 256-byte boundary, and their *_scratch_bytes count 255 bytes
    for it. A view `shift` bytes past a boundary spends 256 - shift of them: at shift = 1 the last carve ends on the scratch's
    last byte (one float too many lands in the back band), at shift = 252 with 251 bytes to spare. Both bands stay intact
    (guarded), and every output has the bits of the same call on an aligned view - both carve from a 256-byte boundary, so
    every product picks the same kernel. (The other three entries use the caller's pointer as it is: not shifted.)"""
    base, got = run(0), run(shift)
    keys = [k for k, v in base.items() if torch.is_tensor(v) and k != "_scratch"]
    assert len(keys) >= 7 and set(keys) == {k for k, v in got.items() if torch.is_tensor(v) and k != "_scratch"}
    for k in keys:
        assert torch.equal(base[k], got[k]), k


# ---- (e) the entries without an operator test ---------------------------------------------------------------------------
def _conc_ref(ps, lang, msk, n_q, nc_v, nfrm, nppf, nsrl, per_vid):
    """x_mul[((q, v), f), (arg, p)] = [ps[(q, v), f * nppf + p] | mask * lang[(q, v | 0), arg]]"""
    QV, dobj, nvl = n_q * nc_v, ps.shape[-1], nc_v if per_vid else 1
    vis = ps.reshape(QV, nfrm, 1, nppf, dobj).expand(QV, nfrm, nsrl, nppf, dobj)
    if lang is None:
        return vis.reshape(-1, dobj)
    lg = lang.reshape(n_q, nvl, nsrl, -1)
    if msk is not None:
        lg = lg * (msk.reshape(n_q, nvl, nsrl, 1) != 0).to(lg.dtype)
    lg = lg.expand(n_q, nc_v, nsrl, lg.shape[-1]).reshape(QV, 1, nsrl, 1, -1).expand(QV, nfrm, nsrl, nppf, lg.shape[-1])
    return torch.cat([vis, lg], -1).reshape(QV * nfrm * nsrl * nppf, -1)


@pytest.mark.parametrize("per_vid", [False, True])
@pytest.mark.parametrize("with_msk", [False, True])
@pytest.mark.parametrize("dlang", [3, 0])
def test_conc_forward_backward(per_vid, with_msk, dlang):
    n_q, nc_v, nfrm, nppf, nsrl, dobj = 2, 3, 2, 5, 4, 7
    g = torch.Generator().manual_seed(11 + dlang)
    nvl = nc_v if per_vid else 1
    ps = torch.randn(n_q * nc_v * nfrm * nppf, dobj, generator=g)
    lang = torch.randn(n_q * nvl * nsrl, dlang, generator=g) if dlang else None
    msk = torch.randint(0, 2, (n_q, nvl, nsrl), generator=g) if with_msk else None
    rows = n_q * nc_v * nfrm * nsrl * nppf
    d_x = torch.randn(rows, dobj + dlang, generator=g)
    psr = ps.to(F64).requires_grad_(True)
    lr = lang.to(F64).requires_grad_(True) if dlang else None
    xm = _conc_ref(psr, lr, msk, n_q, nc_v, nfrm, nppf, nsrl, per_vid)
    (xm * d_x.double()).sum().backward()
    if dlang:                                                        # the forward entry needs a language part
        out = torch.empty(rows, dobj + dlang, dtype=torch.float32, device="cuda")
        mk = msk.cuda().contiguous() if with_msk else None
        psd, ld = dev(ps), dev(lang)
        L.check(L.load().vog_conc_f32_fwd(L.ptr(psd), L.ptr(ld), L.ptr(mk), L.ptr(out), n_q, nc_v, nfrm, nppf, nsrl, dobj, dlang,
                                          1 if per_vid else 0, L.stream_ptr()), "vog_conc_f32_fwd")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().double(), xm.detach())          # a copy: exact
    d_ps, d_lang = bwd.conc_backward(dev(d_x), n_q, nc_v, nfrm, nppf, nsrl, dobj, inds_msk=msk, lang_per_vid=per_vid)
    torch.cuda.synchronize()
    close(d_ps, psr.grad, what="d_ps")
    if dlang:
        close(d_lang, lr.grad, tol=TOL_SUM, what="d_lang")
        if with_msk:
            assert (d_lang.cpu()[msk.reshape(-1) == 0] == 0).all()
    else:
        assert d_lang is None


@pytest.mark.parametrize("M,d,dhead,geo", [(60, 32, 24, G60A), (60, 32, 80, G60B), (60, 9, 70, G60A), (1, 5, 2, (1, 1, 1, 1))])
@pytest.mark.parametrize("need,want_dx", [(None, True), (("lin2.0.weight", "lin2.2.bias"), True), (("lin2.2.weight",), False)])
def test_score_head_forward_backward(M, d, dhead, geo, need, want_dx):
    n_vid, nfrm, nsrl, nppf = geo
    g = torch.Generator().manual_seed(M + d * 5 + dhead)
    p = _tail_params(d, 1, dhead, g)
    names = {"wl": "lin2.0.weight", "bl": "lin2.0.bias", "wl2": "lin2.2.weight", "bl2": "lin2.2.bias"}
    y = torch.randn(M, d, generator=g)
    dmo = torch.randn(n_vid, nsrl, nfrm * nppf, generator=g)
    lv = {k: p[k].to(F64).requires_grad_(True) for k in names}
    yr = y.to(F64).requires_grad_(True)
    logit = torch.relu(yr @ lv["wl"].t() + lv["bl"]) @ lv["wl2"].reshape(-1) + lv["bl2"]
    outs = logit.reshape(n_vid, nfrm, nsrl, nppf).permute(0, 2, 1, 3).reshape(n_vid, nsrl, nfrm * nppf)
    (outs * dmo.double()).sum().backward()
    w = {k: dev(p[k]) for k in names}
    got = torch.empty(n_vid, nsrl, nfrm * nppf, dtype=torch.float32, device="cuda")
    yd = dev(y)
    with guarded(M * dhead * 4) as sc:
        L.check(L.load().vog_score_head_f32(L.ptr(yd), L.ptr(w["wl"]), L.ptr(w["bl"]), L.ptr(w["wl2"]), L.ptr(w["bl2"]), L.ptr(got), L.ptr(sc),
                                            M * dhead * 4, M, d, dhead, n_vid, nfrm, nppf, nsrl, L.stream_ptr()), "vog_score_head_f32")
    close(got, outs, what="mdl_outs")
    sd = {names[k]: w[k] for k in names}
    d_x, gr = score_head_bwd_call(sd, yd, dev(dmo), n_vid, nfrm, nppf, nsrl, need=None if need is None else set(need), want_dx=want_dx)
    assert set(gr) == (set(names.values()) if need is None else set(need)) and (d_x is not None) == want_dx
    for k, nm in names.items():
        if nm in gr:
            close(gr[nm], lv[k].grad, tol=TOL_SUM if k in SUMS else TOL, what=nm)
    if want_dx:
        close(d_x, yr.grad, what="d_x")


def _eval_case(conc, nvl):
    """-> B, nc_v, ncmp, NP, nfrm0, nppf0, nsrl, cmp[r] (the comparison each proposal row belongs to; None: the video's)"""
    B, ncmp, nfrm0, nppf0, nsrl = 3, 2, 4, 5, 6                  # pairwise distinct
    if conc == "temp":
        return B, 1, ncmp, ncmp * nfrm0 * nppf0, nfrm0, nppf0, nsrl, torch.arange(ncmp * nfrm0 * nppf0) // (nfrm0 * nppf0)
    if conc == "spat":
        return B, 1, ncmp, nfrm0 * ncmp * nppf0, nfrm0, nppf0, nsrl, (torch.arange(nfrm0 * ncmp * nppf0) // nppf0) % ncmp
    return B, ncmp, ncmp, nfrm0 * nppf0, nfrm0, nppf0, nsrl, None


@pytest.mark.parametrize("conc,nvl", [("temp", 1), ("spat", 1), ("sep", 1), ("sep", 2)])
@pytest.mark.parametrize("parts", ["both", "no_d_outs", "no_d_eval"])
def test_score_eval_backward(conc, nvl, parts):
    B, nc_v, ncmp, NP, nfrm0, nppf0, nsrl, cmp_of = _eval_case(conc, nvl)
    g = torch.Generator().manual_seed(NP + nvl)
    logits = torch.randn(B, nc_v, nsrl, NP, generator=g)
    d_outs, d_eval = torch.randn(logits.shape, generator=g), torch.randn(logits.shape, generator=g)
    am, cm = torch.randint(0, 2, (B, nvl, nsrl), generator=g), torch.randint(0, 2, (B, ncmp), generator=g)
    assert 0 < int(am.sum()) < am.numel() and 0 < int(cm.sum()) < cm.numel()
    lr = logits.to(F64).requires_grad_(True)
    m_arg = am.double().expand(B, nc_v, nsrl).reshape(B, nc_v, nsrl, 1)
    m_cmp = cm.double()[:, cmp_of].reshape(B, 1, 1, NP) if cmp_of is not None else cm.double().reshape(B, nc_v, 1, 1)
    ev = torch.sigmoid(lr) * m_arg * m_cmp
    loss = (ev * d_eval.double()).sum() * (0 if parts == "no_d_eval" else 1) + (lr * d_outs.double()).sum() * (0 if parts == "no_d_outs" else 1)
    loss.backward()
    out = torch.empty_like(logits, device="cuda")
    lg, do, de, amd, cmd = dev(logits), dev(d_outs), dev(d_eval), am.cuda(), cm.cuda()
    args = (L.ptr(lg), L.ptr(do) if parts != "no_d_outs" else None, L.ptr(de) if parts != "no_d_eval" else None,
            L.ptr(amd), L.ptr(cmd), L.ptr(out), B * nc_v, nsrl, NP, L.CONC_TYPE[conc], ncmp, nc_v, nvl, nfrm0, nppf0)
    L.check(L.load().vog_score_eval_bwd_f32(*args, L.stream_ptr()), "vog_score_eval_bwd_f32")
    torch.cuda.synchronize()
    close(out, lr.grad, what="d_logits")
    if parts == "no_d_eval":
        assert torch.equal(out.cpu(), d_outs)


@pytest.mark.parametrize("conc", ["temp", "spat"])
def test_score_eval_backward_rejects_a_mismatched_NP(conc):
    B, nc_v, ncmp, NP, nfrm0, nppf0, nsrl, _ = _eval_case(conc, 1)
    t = torch.zeros(B * nsrl * (NP + nppf0), device="cuda")
    am, cm = torch.ones(B, 1, nsrl, dtype=torch.int64, device="cuda"), torch.ones(B, ncmp, dtype=torch.int64, device="cuda")
    with pytest.raises(L.VogError, match="rc=-1"):
        L.check(L.load().vog_score_eval_bwd_f32(L.ptr(t), None, L.ptr(t), L.ptr(am), L.ptr(cm), L.ptr(t), B, nsrl, NP + nppf0, L.CONC_TYPE[conc],
                                                ncmp, 1, 1, nfrm0, nppf0, L.stream_ptr()), "vog_score_eval_bwd_f32")
    with pytest.raises(L.VogError, match="rc=-1"):                 # nvl is 1 or nc_v
        L.check(L.load().vog_score_eval_bwd_f32(L.ptr(t), None, L.ptr(t), L.ptr(am), L.ptr(cm), L.ptr(t), B, nsrl, NP, L.CONC_TYPE[conc],
                                                ncmp, 1, 2, nfrm0, nppf0, L.stream_ptr()), "vog_score_eval_bwd_f32")


@pytest.mark.parametrize("rep", [1, 5])
@pytest.mark.parametrize("with_y", [False, True])
def test_rep_sum(rep, with_y):
    M, N, ldx, F, ldy, col0 = 12, 7, 13, 4, 10, 2
    g = torch.Generator().manual_seed(rep)
    x, y = torch.randn(M * rep, ldx, generator=g), torch.randn(M // F, ldy, generator=g)
    ref = x.double()[:, col0:col0 + N].reshape(M, rep, N).sum(1)
    if with_y:
        ref = ref + y.double()[:, 1:1 + N].repeat_interleave(F, 0) / F
    xd, yd = dev(x), dev(y)
    out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    L.check(L.load().vog_rep_sum_f32(bwd._ptr_view(xd, col0), ldx, rep, bwd._ptr_view(yd, 1) if with_y else None, ldy, F if with_y else 0,
                                     L.ptr(out), M, N, L.stream_ptr()), "vog_rep_sum_f32")
    torch.cuda.synchronize()
    close(out, ref, what="rep_sum")


def test_row_mean_and_concat_rows():
    g = torch.Generator().manual_seed(3)
    G, F, N = 5, 7, 9
    x = torch.randn(G * F, N, generator=g)
    out = torch.empty(G, N, dtype=torch.float32, device="cuda")
    xd = dev(x)
    L.check(L.load().vog_row_mean_f32(L.ptr(xd), L.ptr(out), G, F, N, L.stream_ptr()), "vog_row_mean_f32")
    close(out, x.double().reshape(G, F, N).mean(1), what="row_mean")
    M, Na, ra, Nb, rb = 30, 4, 2, 3, 5                             # rep_a != rep_b
    a, b = torch.randn(M // ra, Na, generator=g), torch.randn(M // rb, Nb, generator=g)
    cat = torch.empty(M, Na + Nb, dtype=torch.float32, device="cuda")
    ad, bd = dev(a), dev(b)
    L.check(L.load().vog_concat_rows_f32(L.ptr(ad), Na, ra, L.ptr(bd), Nb, rb, L.ptr(cat), M, L.stream_ptr()), "vog_concat_rows_f32")
    torch.cuda.synchronize()
    assert torch.equal(cat.cpu(), torch.cat([a.repeat_interleave(ra, 0), b.repeat_interleave(rb, 0)], 1))


def test_adam_three_steps_vs_float64():
    n, lr, b1, b2, eps = 1000, 1e-2, 0.9, 0.99, 1e-8                # n % 256 != 0
    g = torch.Generator().manual_seed(8)
    p0 = torch.randn(n, generator=g)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in (1, 2, 3):
        gr = torch.randn(n, generator=g)
        gd = dev(gr)
        L.check(L.load().vog_adam_f32(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), n, lr, b1, b2, eps, step, L.stream_ptr()), "vog_adam_f32")
        torch.cuda.synchronize()
        mr = b1 * mr + (1 - b1) * gr.double()
        vr = b2 * vr + (1 - b2) * gr.double() ** 2
        pr = pr - lr / (1 - b1 ** step) * mr / (vr.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    close(p, pr, what="p"); close(m, mr, what="m"); close(v, vr, what="v")


# ---- (f) argument contracts (no kernel runs) ----------------------------------------------------------------------------
@pytest.mark.parametrize("fn,good", [("vog_mul_tail_bwd_scratch_bytes", (4, 8, 4, 4)), ("vog_attn_f32_scratch_bytes", (2, 6, 3, 8)),
                                     ("vog_linear_f32_scratch_bytes", (4, 8)), ("vog_lang_f32_scratch_bytes", (2, 3, 2, 4, 4, 2, 6, 5)),
                                     ("vog_score_head_f32_bwd_scratch_bytes", (4, 8, 4))])
def test_scratch_bytes_refuse_non_positive_dimensions(fn, good):
    f = getattr(L.load(), fn)
    assert f(*good) > 0
    for i in range(len(good)):
        for bad in (0, -3):
            if fn == "vog_mul_tail_bwd_scratch_bytes" and i == 3 and bad == 0:
                continue                                             # dhead = 0: a tail without the score head
            a = list(good)
            a[i] = bad
            assert f(*a) == -1, (fn, a)
    if fn == "vog_lang_f32_scratch_bytes":
        assert f(2, 3, 2, 4, 4, 5, 6, 5) == -1                       # at most 4 layers


class _ShortBy1:
    """The library with one *_scratch_bytes entry answering a byte too few: the wrapper then allocates and declares nb - 1."""

    def __init__(self, lib, name):
        self._lib, self._name = lib, name

    def __getattr__(self, k):
        f = getattr(self._lib, k)
        return (lambda *a: f(*a) - 1) if k == self._name else f


@pytest.mark.parametrize("entry", ["tail", "attn", "linear", "lang", "score_head_bwd", "score_head"])
def test_entries_refuse_a_scratch_one_byte_short(entry, monkeypatch):
    lib = L.load()
    short = {"tail": "vog_mul_tail_bwd_scratch_bytes", "attn": "vog_attn_f32_scratch_bytes", "linear": "vog_linear_f32_scratch_bytes",
             "lang": "vog_lang_f32_scratch_bytes", "score_head_bwd": "vog_score_head_f32_bwd_scratch_bytes"}.get(entry)
    if short:
        monkeypatch.setattr(bwd.L, "load", lambda: _ShortBy1(lib, short))
    g = torch.Generator().manual_seed(1)
    z = lambda *s: torch.randn(*s, generator=g).cuda()
    with pytest.raises(L.VogError, match="rc=-2"):
        if entry == "tail":
            bwd._tail_call({k: dev(v) for k, v in _tail_params(8, 4, 0, g).items()}, z(4, 8), z(4, 8))
        elif entry == "attn":
            bwd._attn_call({"wq": z(8, 8), "wk": z(8, 8), "wv": z(8, 8)}, None, z(12, 8), 2, 6, 3, 2, None)
        elif entry == "linear":
            bwd.linear_f32(z(4, 8), z(6, 8), z(6), True)
        elif entry == "lang":
            c = _lang_case(1, [2], 4, 4, 1, 6, 5)
            sd, batch = _lang_dev(c)
            bwd.language_backward(sd, batch, c["T"], 1)
        elif entry == "score_head_bwd":
            sd = {"lin2.0.weight": z(4, 8), "lin2.0.bias": z(4), "lin2.2.weight": z(1, 4), "lin2.2.bias": z(1)}
            bwd.score_head_backward(sd, z(6, 8), z(1, 2, 3), 1, 1, 3, 2)
        else:
            M, d, dhead = 6, 8, 4
            sc = torch.empty(M * dhead * 4, dtype=torch.uint8, device="cuda")
            L.check(lib.vog_score_head_f32(L.ptr(z(M, d)), L.ptr(z(dhead, d)), L.ptr(z(dhead)), L.ptr(z(1, dhead)), L.ptr(z(1)), L.ptr(z(1, 2, 3)),
                                           L.ptr(sc), M * dhead * 4 - 1, M, d, dhead, 1, 1, 3, 2, L.stream_ptr()), "vog_score_head_f32")


def test_attention_refuses_bad_head_and_token_counts():
    z = lambda *s: torch.zeros(*s, device="cuda")
    w = {"wq": z(4, 4), "wk": z(4, 4), "wv": z(4, 4)}
    with pytest.raises(L.VogError, match="rc=-1"):
        bwd._attn_call(w, None, z(12, 4), 2, 6, 3, 5, None)          # n_heads = 5 > d = 4
    lib = L.load()
    S, N, n, d = 2, 6, 4, 4                                          # N % n != 0 (the wrapper asserts it too: call the entry)
    nb = int(lib.vog_attn_f32_scratch_bytes(S, N, n, d))
    x, cat, sc = z(S * N, d), z(S * N, d), torch.empty(nb, dtype=torch.uint8, device="cuda")
    a = L.AttnF32Args()
    a.x, a.wq, a.wk, a.wv, a.cat_out = L.ptr(x), L.ptr(w["wq"]), L.ptr(w["wk"]), L.ptr(w["wv"]), L.ptr(cat)
    a.scratch, a.scratch_bytes, a.S, a.N, a.n, a.d, a.n_heads = L.ptr(sc), nb, S, N, n, d, 2
    with pytest.raises(L.VogError, match="rc=-1"):
        L.check(lib.vog_attn_f32(C.byref(a), L.stream_ptr()), "vog_attn_f32")
