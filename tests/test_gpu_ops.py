"""-m gpu: every operator-level entry point of the C ABI against a plain
fp32 torch reference of the same op on the same (already rounded) operands.
Inputs are asymmetric random data (a transposed MFMA operand / C layout cannot
pass). Tolerances are written per test."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import vog_oracle as vo
from tests.gpu_util import L, t16

pytestmark = pytest.mark.gpu
DT = {"bf16": L.VOG_BF16, "f16": L.VOG_F16}


def _lib():
    return L.load()


def _sp():
    return L.stream_ptr()


def _gemm(a, w, bias=None, residual=None, relu=False, rep=1, rows=None, dtype="bf16",
          want16=False, M=None):
    lib = _lib()
    M = M if M is not None else (a.shape[0] if rows is None else rows.numel())
    N, K = w.shape
    g = L.GemmArgs()
    g.a, g.a_is_f32, g.lda = L.ptr(a), int(a.dtype == torch.float32), a.shape[1]
    g.a_rows = L.ptr(rows)
    g.w, g.ldw = L.ptr(w), K
    g.bias, g.residual, g.ldr = L.ptr(bias), L.ptr(residual), N
    c32 = torch.full((M * rep, N), float("nan"), device="cuda")
    c16 = torch.zeros((M * rep, N), dtype=t16(dtype), device="cuda") if want16 else None
    g.c32, g.c16, g.ldc, g.ldc16 = L.ptr(c32), L.ptr(c16), N, N
    g.M, g.N, g.K, g.relu, g.rep, g.dtype = M, N, K, int(relu), rep, DT[dtype]
    L.check(lib.vog_gemm_bias_act(C.byref(g), _sp()), "gemm")
    torch.cuda.synchronize()
    return c32, c16


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", [(800, 256, 2048), (4000, 768, 576), (4000, 2304, 768),
                                   (130, 70, 48), (48, 8192, 512), (52, 256, 2048), (20, 96, 64),
                                   (333, 200, 72), (1, 16, 32)])
def test_gemm_t16_operands(M, N, K, dtype):
    torch.manual_seed(M * 7 + N)
    a = torch.randn(M, K, device="cuda").to(t16(dtype))
    w = (torch.randn(N, K, device="cuda") / math.sqrt(K)).to(t16(dtype))
    bias = torch.randn(N, device="cuda")
    c32, c16 = _gemm(a, w, bias=bias, relu=True, dtype=dtype, want16=True)
    ref = torch.relu(a.float() @ w.float().t() + bias)
    err = (c32 - ref).abs().max().item()
    assert err <= 2e-3 * max(1.0, ref.abs().max().item()), err       # fp32 accumulation order only
    assert (c16.float() - ref).abs().max().item() <= 1e-2 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("M", [40, 160, 800])
def test_gemm_f32_a_residual_rep_gather(M):
    torch.manual_seed(3)
    K, N = 96, 64
    table = torch.randn(500, K, device="cuda")
    rows = torch.randint(0, 500, (M,), device="cuda", dtype=torch.int32)
    w = (torch.randn(N, K, device="cuda") / 8).to(torch.float16)
    c32, _ = _gemm(table, w, rows=rows, dtype="f16")
    ref = table[rows.long()].half().float() @ w.float().t()
    assert (c32 - ref).abs().max().item() <= 2e-3
    # residual
    a = torch.randn(M, K, device="cuda")
    res = torch.randn(M, N, device="cuda")
    c32, _ = _gemm(a, w, residual=res, dtype="f16")
    ref = a.half().float() @ w.float().t() + res
    assert (c32 - ref).abs().max().item() <= 2e-3
    # row replication (segment feature broadcast onto the frame's proposals)
    c32, c16 = _gemm(a, w, rep=5, dtype="f16", want16=True)
    ref = (a.half().float() @ w.float().t()).repeat_interleave(5, dim=0)
    assert (c32 - ref).abs().max().item() <= 2e-3
    assert (c16.float() - ref).abs().max().item() <= 2e-2


def frag_index(N, dp, kind):
    """Flat offsets of (token i, column dd) inside one (sequence, head) block of the
    fragment-ordered q/k ('qk') or v ('v') layout (csrc/common.h frag_qk / frag_v)."""
    i = torch.arange(N).view(N, 1)
    dd = torch.arange(dp).view(1, dp)
    if kind == "qk":
        return ((i >> 5) * (dp >> 4) + (dd >> 4)) * 512 + ((((dd >> 3) & 1) << 5) + (i & 31)) * 8 + (dd & 7)
    kl = i & 31
    r = kl & 15
    j = ((r >> 3) << 2) + (r & 3)
    hi = (r >> 2) & 1
    return ((((i >> 5) * (dp >> 5) + (dd >> 5)) * 2 + (kl >> 4)) * 64 + (hi << 5) + (dd & 31)) * 8 + j


def to_frag(x, kind):
    """[S,H,N,dp] row-major -> [S,H,npad*dp] fragment order (pad tokens zero)."""
    S, H, N, dp = x.shape
    npad = (N + 31) // 32 * 32
    idx = frag_index(N, dp, kind).reshape(-1).to(x.device)
    assert idx.unique().numel() == N * dp and int(idx.max()) < npad * dp
    out = torch.zeros(S, H, npad * dp, dtype=x.dtype, device=x.device)
    out[:, :, idx] = x.reshape(S, H, N * dp)
    return out


def from_frag(f, N, dp, kind):
    idx = frag_index(N, dp, kind).reshape(-1).to(f.device)
    S, H = f.shape[:2]
    return f[:, :, idx].reshape(S, H, N, dp)


@pytest.mark.parametrize("M,N,K", [(48, 8192, 2048), (52, 256, 2048), (20, 2304, 256), (7, 32, 64)])
def test_gemm_skinny_fragment_ordered_weights(M, N, K):
    import numpy as np
    lib = _lib()
    torch.manual_seed(M + N)
    a = torch.randn(M, K, device="cuda")
    w = (torch.randn(N, K) / math.sqrt(K)).contiguous()
    wf = np.zeros(N * K, np.uint16)
    wn = w.numpy()
    L.check(lib.vog_pack_w_frag(wn.ctypes.data, K, N, K, wf.ctypes.data, L.VOG_F16), "pack")
    wfd = torch.from_numpy(wf.view(np.int16)).cuda()
    bias = torch.randn(N, device="cuda")
    g = L.GemmArgs()
    g.a, g.a_is_f32, g.lda, g.w, g.ldw, g.w_frag = L.ptr(a), 1, K, L.ptr(wfd), K, 1
    c32 = torch.full((M, N), float("nan"), device="cuda")
    g.bias, g.c32, g.ldc, g.M, g.N, g.K, g.relu, g.rep, g.dtype = L.ptr(bias), L.ptr(c32), N, M, N, K, 1, 1, L.VOG_F16
    L.check(lib.vog_gemm_bias_act(C.byref(g), _sp()), "gemm")
    torch.cuda.synchronize()
    ref = torch.relu(a.half().float() @ w.cuda().half().float().t() + bias)
    assert (c32 - ref).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("M,N,K", [(48, 8192, 2048), (52, 256, 2048), (20, 96, 64)])
def test_gemm_skinny_fragment_ordered_activations(M, N, K):
    """a_frag: A in [m/16][K/32][lane][8] order (what vog_bilstm_step writes with out_frag)."""
    lib = _lib()
    torch.manual_seed(M + N + 1)
    a = torch.randn(M, K, device="cuda").half()
    w = (torch.randn(N, K, device="cuda") / math.sqrt(K)).half()
    m = torch.arange(M, device="cuda").view(-1, 1)
    k = torch.arange(K, device="cuda").view(1, -1)
    idx = ((((m >> 4) * (K >> 5) + (k >> 5)) * 64) + (((k >> 3) & 3) << 4) + (m & 15)) * 8 + (k & 7)
    mp = (M + 15) // 16 * 16
    af = torch.zeros(mp * K, dtype=torch.float16, device="cuda")
    af[idx.reshape(-1)] = a.reshape(-1)
    bias = torch.randn(N, device="cuda")
    g = L.GemmArgs()
    g.a, g.a_is_f32, g.lda, g.w, g.ldw, g.a_frag = L.ptr(af), 0, K, L.ptr(w), K, 1
    c32 = torch.full((M, N), float("nan"), device="cuda")
    g.bias, g.c32, g.ldc, g.M, g.N, g.K, g.relu, g.rep, g.dtype = L.ptr(bias), L.ptr(c32), N, M, N, K, 0, 1, L.VOG_F16
    L.check(lib.vog_gemm_bias_act(C.byref(g), _sp()), "gemm")
    torch.cuda.synchronize()
    ref = a.float() @ w.float().t() + bias
    assert (c32 - ref).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())
    g.M = 100   # not the M <= 64 kernel: must be refused, not silently misread
    assert lib.vog_gemm_bias_act(C.byref(g), _sp()) != 0


@pytest.mark.parametrize("M,N,K,splits,rep", [(800, 256, 2048, 8, 1), (160, 256, 3072, 12, 5), (130, 64, 256, 3, 1)])
def test_gemm_splitk_and_finish(M, N, K, splits, rep):
    lib = _lib()
    torch.manual_seed(M + splits)
    a = torch.randn(M, K, device="cuda").half()
    w = (torch.randn(N, K, device="cuda") / math.sqrt(K)).half()
    bias = torch.randn(N, device="cuda")
    slabs = torch.full((splits, M, N), float("nan"), device="cuda")
    g = L.GemmArgs()
    g.a, g.a_is_f32, g.lda, g.w, g.ldw = L.ptr(a), 0, K, L.ptr(w), K
    g.c32, g.ldc, g.M, g.N, g.K, g.rep, g.dtype, g.splitk = L.ptr(slabs), N, M, N, K, 1, L.VOG_F16, splits
    L.check(lib.vog_gemm_bias_act(C.byref(g), _sp()), "splitk gemm")
    out32 = torch.full((M * rep, N + 8), float("nan"), device="cuda")
    out16 = torch.zeros((M * rep, N + 8), dtype=torch.bfloat16, device="cuda")
    f = L.SplitkProb()
    f.slabs, f.splits, f.M, f.N, f.bias, f.relu, f.rep = L.ptr(slabs), splits, M, N, L.ptr(bias), 1, rep
    f.c32, f.c16, f.ldc, f.ldc16, f.c16_dtype = L.ptr(out32), L.ptr(out16), N + 8, N + 8, L.VOG_BF16
    L.check(lib.vog_splitk_finish(C.byref(f), None, _sp()), "finish")
    torch.cuda.synchronize()
    ref = torch.relu(a.float() @ w.float().t() + bias).repeat_interleave(rep, dim=0)
    assert (out32[:, :N] - ref).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(out16[:, :N], out32[:, :N].to(torch.bfloat16))
    assert torch.isnan(out32[:, N:]).all()


def _attn_ref(q, k, v, u, peb, n_box, inv_scale, use_rel):
    """q,k,v [S,H,N,dh] fp32 (already rounded); u [S,N,H]"""
    logits = q @ k.transpose(-1, -2)
    if use_rel:
        ub = u.permute(0, 2, 1)                                # [S,H,N]
        bias = torch.relu(ub.unsqueeze(-1) - ub.unsqueeze(-2) + peb.view(1, -1, 1, 1))
        logits = logits + bias
    p = torch.softmax(logits * inv_scale, dim=-1)
    return p @ v


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("S,N,H,dh,dp,nsrl,use_rel", [
    (40, 100, 3, 256, 256, 5, 1), (4, 200, 3, 171, 192, 1, 1), (6, 25, 3, 256, 256, 5, 1),
    (3, 140, 3, 11, 32, 1, 1), (2, 700, 2, 64, 64, 1, 0), (5, 50, 3, 100, 128, 2, 1),
    (2, 33, 1, 16, 32, 1, 1),
    # more than 8 key blocks, fewer than 512 tokens -> attn_frag_kernel (tests/golden/attn_plans.json)
    (2, 300, 2, 64, 64, 1, 1),
    # long sequences -> shared-tile kernel (K/V blocks through LDS-DMA, 128 queries per workgroup)
    (2, 1000, 3, 128, 128, 5, 1), (1, 2011, 3, 171, 192, 1, 1), (3, 520, 2, 100, 128, 2, 1),
    (9, 640, 1, 32, 32, 1, 1)])
def test_rel_attention(S, N, H, dh, dp, nsrl, use_rel, dtype):
    lib = _lib()
    torch.manual_seed(S * 1000 + N)
    td = t16(dtype)
    npad = (N + 31) // 32 * 32
    q = torch.zeros(S, H, N, dp, device="cuda")
    k = torch.zeros(S, H, N, dp, device="cuda")
    v = torch.zeros(S, H, N, dp, device="cuda")
    q[..., :dh] = torch.randn(S, H, N, dh, device="cuda") * 2
    k[..., :dh] = torch.randn(S, H, N, dh, device="cuda") * 2
    v[..., :dh] = torch.randn(S, H, N, dh, device="cuda")
    q16, k16, v16 = q.to(td), k.to(td), v.to(td)
    qf, kf, vf = to_frag(q16, "qk"), to_frag(k16, "qk"), to_frag(v16, "v")
    # pad keys: K may hold anything (masked); V pad must be finite (contract)
    n_box = N // nsrl
    NP = n_box                      # one sequence per "video" here
    u_box = torch.randn(S, n_box, H, device="cuda") * 3
    peb = torch.randn(H, device="cuda")
    out = torch.full((S * N, H * dp), float("nan"), device="cuda").to(td)
    inv_scale = 1.0 / math.sqrt(H * dh)
    a = L.AttnArgs()
    a.q, a.k, a.vt, a.out16 = L.ptr(qf), L.ptr(kf), L.ptr(vf), L.ptr(out)
    a.u, a.pe_b = L.ptr(u_box.contiguous()), L.ptr(peb)
    a.S, a.N, a.H, a.dp, a.npad = S, N, H, dp, npad
    a.use_rel, a.n_box, a.seq_per_vid, a.NP = use_rel, n_box, 1, NP
    a.inv_scale, a.dtype = inv_scale, DT[dtype]
    L.check(lib.vog_rel_attention_fwd(C.byref(a), _sp()), "attn")
    torch.cuda.synchronize()
    u_tok = u_box.repeat(1, nsrl, 1)                            # token j -> box j % n_box
    ref = _attn_ref(q16.float(), k16.float(), v16.float(), u_tok, peb,
                    n_box, inv_scale, use_rel)                  # [S,H,N,dp]
    got = out.float().view(S, N, H, dp).permute(0, 2, 1, 3)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    tol = (2.5e-2 if dtype == "bf16" else 4e-3) * max(1.0, ref.abs().max().item())
    assert err <= tol, (err, tol)
    assert (got[..., dh:] == 0).all()                           # padded head columns stay zero


@pytest.mark.parametrize("S,N,H,dh,dp,nsrl,use_rel", [
    (1, 2011, 3, 171, 192, 1, 1), (2, 1100, 3, 128, 128, 5, 1), (1, 4000, 1, 171, 192, 1, 1),
    (3, 1024, 2, 64, 64, 1, 0), (2, 1057, 1, 32, 32, 1, 1)])
@pytest.mark.parametrize("hostile", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_rel_attention_long_fixed_reference(S, N, H, dh, dp, nsrl, use_rel, hostile, dtype):
    """Long sequences with a guard flag -> attn_tile2_kernel (csrc/attn_tile2_dev.h): softmax against
    the row maximum of key block 0. hostile = 1 plants keys far above anything in block 0 (logits +60
    and more): the kernel must raise the flag and the running-maximum pass must produce the result."""
    lib = _lib()
    torch.manual_seed(S * 1000 + N + hostile)
    td = t16(dtype)
    npad = (N + 31) // 32 * 32
    q = torch.zeros(S, H, N, dp, device="cuda")
    k = torch.zeros(S, H, N, dp, device="cuda")
    v = torch.zeros(S, H, N, dp, device="cuda")
    q[..., :dh] = torch.randn(S, H, N, dh, device="cuda") * 2
    k[..., :dh] = torch.randn(S, H, N, dh, device="cuda") * 2
    v[..., :dh] = torch.randn(S, H, N, dh, device="cuda")
    inv_scale = 1.0 / math.sqrt(H * dh)
    if hostile:
        # a few late keys aligned with a few queries: q.k * inv_scale ~ +100 nats above block 0's logits
        for j, i in ((N - 5, 3), (N // 2 + 1, 40), (700, N - 1)):
            k[:, :, j, :dh] = q[:, :, i, :dh] * (100.0 / inv_scale) / (q[:, :, i, :dh] ** 2).sum(-1, keepdim=True)
    q16, k16, v16 = q.to(td), k.to(td), v.to(td)
    qf, kf, vf = to_frag(q16, "qk"), to_frag(k16, "qk"), to_frag(v16, "v")
    n_box = N // nsrl
    u_box = torch.randn(S, n_box, H, device="cuda") * 3
    peb = torch.randn(H, device="cuda")
    u_tok = u_box.repeat(1, nsrl, 1)
    if N % nsrl:
        u_tok = torch.cat([u_tok, u_box[:, : N - n_box * nsrl]], 1)
    ref = _attn_ref(q16.float(), k16.float(), v16.float(), u_tok, peb, n_box, inv_scale, use_rel)
    flag = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    outs = []
    for guard in (None, flag):
        out = torch.full((S * N, H * dp), float("nan"), device="cuda").to(td)
        a = L.AttnArgs()
        a.q, a.k, a.vt, a.out16 = L.ptr(qf), L.ptr(kf), L.ptr(vf), L.ptr(out)
        a.u, a.pe_b = L.ptr(u_box.contiguous()), L.ptr(peb)
        a.S, a.N, a.H, a.dp, a.npad = S, N, H, dp, npad
        a.use_rel, a.n_box, a.seq_per_vid, a.NP = use_rel, n_box, 1, n_box
        a.inv_scale, a.dtype = inv_scale, DT[dtype]
        a.guard_flag = L.ptr(guard) if guard is not None else None
        L.check(lib.vog_rel_attention_fwd(C.byref(a), _sp()), "attn")
        torch.cuda.synchronize()
        got = out.float().view(S, N, H, dp).permute(0, 2, 1, 3)
        assert torch.isfinite(got).all()
        err = (got - ref).abs().max().item()
        tol = 2.5e-2 * max(1.0, ref.abs().max().item())
        assert err <= tol, (guard is not None, err, tol)
        assert (got[..., dh:] == 0).all()
        outs.append(got)
    if dtype == "bf16" or hostile:
        assert int(flag[0].item()) == (1 if hostile else 0)      # raised exactly when the reference moved too far
    # (f16 trips 13 nats above block 0's maximum instead of 28: the 3-4 nats of logit spread of the small-head cases here
    #  may or may not get there - either way the result above was checked)
    assert (flag[1:] == 7).all()
    if hostile:
        assert torch.equal(outs[0], outs[1])                     # the fallback pass is the running-maximum kernel


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_qkv_layout(dtype):
    lib = _lib()
    torch.manual_seed(5)
    S, N, H, d = 3, 37, 3, 32
    heads = vo.chunk_sizes(d, H)                                # 11, 11, 10
    dp, npad = 32, 64
    td = t16(dtype)
    x = torch.randn(S * N, d, device="cuda").to(td)
    wq, wk, wv = (torch.randn(d, d, device="cuda") / 6 for _ in range(3))
    wpad = torch.zeros(3 * H * dp, d, device="cuda")
    off = 0
    for h, dh in enumerate(heads):
        for which, w in enumerate((wq, wk, wv)):
            wpad[(which * H + h) * dp:(which * H + h) * dp + dh] = w[off:off + dh]
        off += dh
    wpad = wpad.to(td)
    q = torch.zeros((S, H, npad * dp), device="cuda").to(td)
    k = torch.zeros((S, H, npad * dp), device="cuda").to(td)
    vt = torch.zeros((S, H, npad * dp), device="cuda").to(td)
    a = L.QkvArgs()
    a.x16, a.ldx, a.wqkv, a.ldw = L.ptr(x), d, L.ptr(wpad), d
    a.q, a.k, a.vt = L.ptr(q), L.ptr(k), L.ptr(vt)
    a.S, a.N, a.H, a.dp, a.npad, a.K, a.dtype = S, N, H, dp, npad, d, DT[dtype]
    L.check(lib.vog_qkv_proj(C.byref(a), _sp()), "qkv")
    torch.cuda.synchronize()
    full = (x.float() @ wpad.float().t()).view(S, N, 3, H, dp)
    tol = 2e-2
    for which, (buf, kind) in enumerate(((q, "qk"), (k, "qk"), (vt, "v"))):
        got = from_frag(buf.float(), N, dp, kind)
        ref = full[:, :, which].permute(0, 2, 1, 3)
        assert (got - ref).abs().max().item() <= tol, which
        # nothing outside the N*dp valid slots was touched
        msk = torch.ones(npad * dp, dtype=torch.bool, device="cuda")
        msk[frag_index(N, dp, kind).reshape(-1).cuda()] = False
        assert (buf[:, :, msk] == 0).all()


@pytest.mark.parametrize("nppf,nsrl,dp,H", [(20, 5, 256, 3), (5, 5, 64, 3), (7, 5, 32, 2)])
def test_qkv_combine_structured(nppf, nsrl, dp, H):
    """vog_qkv_combine == dense projection of the [vis || lang] token matrix."""
    lib = _lib()
    torch.manual_seed(9)
    n_vid, nfrm = 3, 4
    N = nsrl * nppf
    npad = (N + 31) // 32 * 32
    ncol = 3 * H * dp
    pv = torch.randn(n_vid * nfrm * nppf, ncol, device="cuda")
    pl = torch.randn(n_vid * nsrl, ncol, device="cuda")
    q = torch.zeros(n_vid * nfrm, H, npad * dp, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros_like(q)
    vt = torch.zeros_like(q)
    a = L.QkvCombArgs()
    a.pv, a.pl, a.q, a.k, a.vt = L.ptr(pv), L.ptr(pl), L.ptr(q), L.ptr(k), L.ptr(vt)
    a.n_vid, a.nfrm, a.nppf, a.nsrl, a.H, a.dp, a.npad = n_vid, nfrm, nppf, nsrl, H, dp, npad
    a.lang_per_vid, a.nc_v, a.dtype = 1, 1, L.VOG_BF16
    L.check(lib.vog_qkv_combine(C.byref(a), _sp()), "combine")
    torch.cuda.synchronize()
    # token (s=(v,f), j=a*nppf+p) = PV[v, f*nppf+p] + PL[v, a]
    pvr = pv.view(n_vid, nfrm, 1, nppf, 3, H, dp)
    plr = pl.view(n_vid, 1, nsrl, 1, 3, H, dp)
    tok = (pvr + plr).reshape(n_vid * nfrm, N, 3, H, dp)
    for which, (buf, kind) in enumerate(((q, "qk"), (k, "qk"), (vt, "v"))):
        got = from_frag(buf.float(), N, dp, kind)
        ref = tok[:, :, which].permute(0, 2, 1, 3)
        assert torch.equal(got, ref.to(torch.bfloat16).float()), which


def test_qkv_proj_structured_fused():
    """vog_qkv_proj with pl: visual rows x W[:, :dv]^T + pl[arg], fanned out over the args,
    straight into fragment order == dense projection of the [vis || lang] tokens."""
    lib = _lib()
    torch.manual_seed(11)
    n_vid, nfrm, nppf, nsrl, H, dp, dv, dl = 2, 10, 20, 5, 3, 256, 512, 256
    d = dv + dl
    N = nsrl * nppf
    npad = (N + 31) // 32 * 32
    ncol = 3 * H * dp
    td = torch.bfloat16
    vis = torch.randn(n_vid * nfrm * nppf, dv, device="cuda").to(td)
    lang = torch.randn(n_vid * nsrl, dl, device="cuda")
    w = (torch.randn(ncol, d, device="cuda") / math.sqrt(d)).to(td)
    pl = (lang.to(td).float() @ w[:, dv:].float().t()).contiguous()
    S = n_vid * nfrm
    q = torch.zeros(S, H, npad * dp, dtype=td, device="cuda")
    k = torch.zeros_like(q)
    vt = torch.zeros_like(q)
    a = L.QkvArgs()
    a.x16, a.ldx, a.wqkv, a.ldw = L.ptr(vis), dv, L.ptr(w), d
    a.q, a.k, a.vt = L.ptr(q), L.ptr(k), L.ptr(vt)
    a.S, a.N, a.H, a.dp, a.npad, a.K, a.dtype = S, N, H, dp, npad, dv, L.VOG_BF16
    a.pl, a.nsrl, a.nppf, a.nfrm, a.lang_per_vid, a.nc_v = L.ptr(pl), nsrl, nppf, nfrm, 1, 1
    L.check(lib.vog_qkv_proj(C.byref(a), _sp()), "qkv structured")
    torch.cuda.synchronize()
    pv = (vis.float() @ w[:, :dv].float().t()).view(n_vid, nfrm, 1, nppf, 3, H, dp)
    tok = (pv + pl.view(n_vid, 1, nsrl, 1, 3, H, dp)).reshape(S, N, 3, H, dp)
    for which, (buf, kind) in enumerate(((q, "qk"), (k, "qk"), (vt, "v"))):
        got = from_frag(buf.float(), N, dp, kind)
        ref = tok[:, :, which].permute(0, 2, 1, 3)
        assert (got - ref).abs().max().item() <= 3e-2 * max(1.0, ref.abs().max().item()), which


def _pack32_cols(lib, w32, K, dtype):
    """vog_pack_w_frag32 of the first K columns of the fp32 matrix w32 -> device halfwords."""
    wc = w32.detach().cpu().contiguous()
    N = wc.shape[0]
    dst = torch.empty(N * K, dtype=torch.int16)
    L.check(lib.vog_pack_w_frag32(L.ptr(wc), wc.shape[1], N, K, L.ptr(dst), DT[dtype]), "pack32")
    return dst.cuda()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["obj", "mul", "vis", "obj_p100", "obj_big_ragged"])
def test_qkv_rowblock_equals_tiled(dtype, case):
    """vog_qkv_proj with wqkv_p32 (row-block kernel, csrc/qkvrb_dev.h) writes the same Q/K/V^T fragment
    images as the tiled LDS-DMA GEMM (to the rounding of a different fp32 summation order) and touches
    no pad slot: ragged row counts, K = 512 / 768, and the visual-rows form of mul_tx layer 0 (first
    d_vis columns of a wider weight matrix, 20 tokens per sequence)."""
    lib = _lib()
    torch.manual_seed(23)
    td = t16(dtype)
    # (>= 8192 rows: the all-columns form, QkvRowAllBody - obj_p100 takes its register / 16-byte fragment stores (4000 tokens
    # per sequence: 16-token groups never straddle one), obj_big_ragged the shared V^T writer (203 tokens, ragged last block))
    S, N, H, dp, K, ld = {"obj": (3, 203, 3, 192, 512, 512), "mul": (7, 100, 3, 256, 768, 768),
                          "vis": (13, 20, 3, 256, 512, 768), "obj_p100": (4, 4000, 3, 192, 512, 512),
                          "obj_big_ragged": (41, 203, 3, 192, 512, 512)}[case]
    npad = (N + 31) // 32 * 32
    ncol = 3 * H * dp
    assert lib.vog_qkv_rowblock_supported(ncol, K) == 1
    w32 = (torch.randn(ncol, ld) / math.sqrt(ld)).to(td).float()
    w16 = w32.cuda().to(td)
    wp = _pack32_cols(lib, w32, K, dtype)
    x = torch.randn(S * N, K, device="cuda").to(td)
    outs = []
    for lean in (0, 1):
        q = torch.zeros(S, H, npad * dp, device="cuda").to(td)
        k = torch.zeros_like(q)
        vt = torch.zeros_like(q)
        a = L.QkvArgs()
        a.x16, a.ldx, a.wqkv, a.ldw = L.ptr(x), K, L.ptr(w16), ld
        a.q, a.k, a.vt = L.ptr(q), L.ptr(k), L.ptr(vt)
        a.S, a.N, a.H, a.dp, a.npad, a.K, a.dtype = S, N, H, dp, npad, K, DT[dtype]
        a.wqkv_p32 = L.ptr(wp) if lean else None
        L.check(lib.vog_qkv_proj(C.byref(a), _sp()), "qkv")
        torch.cuda.synchronize()
        outs.append((q, k, vt))
    for name, kind, t, r in zip("qkv", ("qk", "qk", "v"), outs[0], outs[1]):
        d = (t.float() - r.float()).abs().max().item()
        scale = max(1.0, t.float().abs().max().item())
        assert d <= (2e-2 if dtype == "bf16" else 3e-3) * scale, (name, d)
        msk = torch.ones(npad * dp, dtype=torch.bool, device="cuda")
        msk[frag_index(N, dp, kind).reshape(-1).cuda()] = False
        assert (r[:, :, msk] == 0).all(), name
    # and against the dense product
    full = (x.float() @ w16[:, :K].float().t()).view(S, N, 3, H, dp)
    for which, (buf, kind) in enumerate(zip(outs[1], ("qk", "qk", "v"))):
        got = from_frag(buf.float(), N, dp, kind)
        ref = full[:, :, which].permute(0, 2, 1, 3)
        assert (got - ref).abs().max().item() <= 3e-2 * max(1.0, ref.abs().max().item()), which


def test_layernorm():
    lib = _lib()
    torch.manual_seed(1)
    for rows, d in ((4000, 768), (801, 512), (7, 48), (5, 32)):
        x = torch.randn(rows, d, device="cuda") * 3 + 1
        g = torch.randn(d, device="cuda")
        b = torch.randn(d, device="cuda")
        y32 = torch.empty_like(x)
        y16 = torch.empty(rows, d, dtype=torch.bfloat16, device="cuda")
        L.check(lib.vog_residual_layernorm(L.ptr(x), L.ptr(g), L.ptr(b), L.ptr(y32), L.ptr(y16),
                                           rows, d, L.VOG_BF16, _sp()), "ln")
        torch.cuda.synchronize()
        ref = torch.nn.functional.layer_norm(x, (d,), g, b, 1e-5)
        assert (y32 - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item()) + 2e-5
        assert torch.equal(y16, y32.to(torch.bfloat16))


def test_box_u_and_bias_identity():
    """u-form of the bias == the reference's Linear(5,H) on box differences."""
    lib = _lib()
    torch.manual_seed(2)
    n, H = 200, 3
    props = torch.rand(n, 7, device="cuda") * torch.tensor([2880., 405, 2880, 405, 9, 400, 1], device="cuda")
    w = torch.randn(H, 5, device="cuda")
    b = torch.randn(H, device="cuda")
    u = torch.empty(n, H, device="cuda")
    L.check(lib.vog_box_u(L.ptr(props), L.ptr(w), L.ptr(u), n, H, 720.0, 405.0, 10.0, _sp()), "box_u")
    torch.cuda.synchronize()
    bx = vo.normalise_boxes(props[:, :5].cpu(), 720.0, 405.0, 10.0)
    for h in range(H):
        ref = vo.box_bias_head(bx.unsqueeze(0), w[h].cpu(), b[h].cpu())[0]
        got = torch.relu(u[:, h].cpu().unsqueeze(1) - u[:, h].cpu().unsqueeze(0) + b[h].cpu())
        assert (got - ref).abs().max().item() <= 2e-5


def test_srl_gather_and_argvec():
    lib = _lib()
    from oracle import cases
    cfg, sd, batch, c = cases.build("small/vog_sep")
    words = torch.from_numpy(batch["srl_arg_words_ind"]).cuda()
    mask = torch.from_numpy(batch["srl_arg_word_mask"]).cuda()
    B, nv = words.shape[:2]
    T = int(batch["srl_arg_word_mask_len"].max())
    tok = torch.empty(B * nv, T, dtype=torch.int32, device="cuda")
    keep = mask.clone()
    L.check(lib.vog_srl_gather(L.ptr(words), L.ptr(mask), L.ptr(tok), B * nv, T, 5, 20, c["vocab"], _sp()), "g")
    torch.cuda.synchronize()
    ref = vo.srl_arg_seq_to_sent_seq(words.cpu(), mask.cpu(), c["vocab"])[:, :T]
    assert torch.equal(tok.cpu().long(), ref)
    assert torch.equal(keep, mask)
    Ld = 16
    full = torch.randn(B * nv * T, Ld, device="cuda")
    cap = torch.from_numpy(batch["srl_arg_words_capture"]).cuda()
    msk = torch.from_numpy(batch["srl_arg_inds_msk"]).cuda()
    w = torch.randn(Ld, 2 * Ld, device="cuda")
    bb = torch.randn(Ld, device="cuda")
    lang = torch.empty(B * nv, 5, Ld, device="cuda")
    L.check(lib.vog_srl_argvec(L.ptr(full), L.ptr(cap), L.ptr(msk), L.ptr(w), L.ptr(bb), L.ptr(lang),
                               B * nv, T, 5, Ld, _sp()), "argvec")
    torch.cuda.synchronize()
    sdd = {"srl_arg_words_out_enc.0.weight": w.cpu(), "srl_arg_words_out_enc.0.bias": bb.cpu()}
    ref = vo.retrieve_srl_args(full.cpu().view(B * nv, T, Ld), cap.cpu(), msk.cpu(), sdd)
    assert (lang.cpu().view_as(ref) - ref).abs().max().item() <= 1e-5


@pytest.mark.parametrize("conc", ["spat", "temp", "sep"])
@pytest.mark.parametrize("np0", [5, 100])
def test_pred_head_exact(conc, np0):
    """Integer/index work: bit-exact against the oracle head, ties included (np0 = 100: the wave-per-item
    form of the p100 shapes, ties across more than one lane round)."""
    lib = _lib()
    torch.manual_seed(4)
    B, ncmp, nsrl, nf = 3, 4, 5, 10
    oc = vo.OracleCfg(conc_type=conc, nppf0=np0)
    if conc == "sep":
        ev = torch.rand(B, ncmp, nsrl, nf * np0)
        props = torch.rand(B, ncmp, nf * np0, 7)
    else:
        ev = torch.rand(B, 1, nsrl, ncmp * nf * np0)
        props = torch.rand(B, ncmp * nf * np0, 7)
    ev[0, 0, 4] = 0.0                         # masked argument: all ties -> first index
    ev[1, 0, 1, :7] = 0.5                     # exact ties inside a frame
    if np0 > 64:
        ev[2, 0, 2, :np0] = 0.25                # a whole frame of ties (more than one round of lanes)
        ev[2, 0, 2, 70] = 0.75; ev[2, 0, 2, 3] = 0.75   # the maximum twice: lane 6 (second round) and lane 3
    fin = torch.rand(B, ncmp)
    out = {"mdl_outs_eval": ev, "fin_scores": fin}
    inp = {"pad_proposals": props, "new_srl_idxs": torch.zeros(B, ncmp, dtype=torch.int64)}
    ref = vo.pred_head(oc, out, inp)
    rb = int(lib.vog_pred_record_bytes(ncmp, nsrl, nf))
    rec = torch.empty(B, rb // 4, device="cuda")
    a = L.PredArgs()
    evd, prd, find = ev.cuda(), props.cuda(), fin.cuda()
    a.outs_eval, a.props, a.fin_scores, a.rec = L.ptr(evd), L.ptr(prd), L.ptr(find), L.ptr(rec)
    a.B, a.ncmp, a.nsrl, a.nfrm0, a.nppf0, a.conc_type = B, ncmp, nsrl, nf, np0, L.CONC_TYPE[conc]
    L.check(lib.vog_pred_head(C.byref(a), _sp()), "pred")
    torch.cuda.synchronize()
    nb = nsrl * ncmp * nf
    r = rec.cpu()
    assert torch.equal(r[:, : nb * 7].reshape(B, nsrl, ncmp, nf, 7), ref["boxes"])
    assert torch.equal(r[:, nb * 7: nb * 8].reshape(B, nsrl, ncmp, nf), ref["scores"])
    idx = r[:, nb * 8:].contiguous().view(torch.int64).reshape(B, nsrl, nf)
    if conc == "temp":
        assert (idx == 0).all()
    else:
        assert torch.equal(idx, ref["indexs"])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("S,nfrm,nsrl,nppf,H,dh,dp,use_rel,lpv", [
    (8, 4, 5, 20, 3, 128, 128, 1, 0), (6, 3, 5, 7, 3, 16, 32, 1, 1), (4, 2, 5, 100, 2, 100, 128, 1, 0),
    (4, 4, 3, 40, 1, 64, 64, 0, 0), (2, 1, 5, 400, 2, 128, 128, 1, 0),
    # head dim 256 (mul_tx at full size): the E x F kernel of attn_struct_ef_dev.h (qvis = 1, several key blocks) with 13 / 4 /
    # 2 key blocks, a partial last proposal block, language rows per video, no bias, fewer than 5 arguments
    (3, 3, 5, 400, 3, 256, 256, 1, 0), (4, 2, 5, 100, 3, 256, 256, 1, 1), (2, 2, 4, 50, 2, 250, 256, 0, 0),
    # two key blocks whose LDS ring (155 904 B with 8 language rows at head dim 256) passes the 150 KB limit -> attn_struct_kernel
    (2, 2, 8, 40, 1, 256, 256, 1, 0)])
@pytest.mark.parametrize("qvis", [0, 1])
def test_rel_attention_struct_equals_full_attention(S, nfrm, nsrl, nppf, H, dh, dp, use_rel, lpv, dtype, qvis):
    """Separable mul_tx layer-0 attention: token (a, p) has k = Kv[p] + Kl[a], v = Vv[p] + Vl[a]; the
    softmax over all nsrl*nppf keys must equal softmax_p'(.)Vv + softmax_a'(.)Vl."""
    _struct_attention_case(S, nfrm, nsrl, nppf, H, dh, dp, use_rel, lpv, dtype, qvis, 1.0)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("spread", [3.0, 5.0])
@pytest.mark.parametrize("S,nfrm,nsrl,nppf,H,dh,dp,use_rel,lpv", [(3, 3, 5, 400, 3, 256, 256, 1, 0), (4, 2, 5, 100, 3, 256, 256, 1, 1)])
def test_rel_attention_struct_ef_large_logit_spread(S, nfrm, nsrl, nppf, H, dh, dp, use_rel, lpv, dtype, spread):
    """the E x F factorisation shifts by mA[p] + mB[a], which can sit far above a row's true maximum (a key weak in
    A = Qv.Kv + bias but dominant through B = Ql.Kv). Queries / keys scaled so that the logits spread over 5 (x 3) to 15 (x 5)
    nats of standard deviation - rows whose winner lies > 17 nats under the shift exist - must still match the full softmax:
    E carries a factor 2^12 that cancels in the quotient (attn_struct_ef_dev.h, EF_ESHIFT)."""
    _struct_attention_case(S, nfrm, nsrl, nppf, H, dh, dp, use_rel, lpv, dtype, 1, spread)


def _struct_attention_case(S, nfrm, nsrl, nppf, H, dh, dp, use_rel, lpv, dtype, qvis, spread):
    lib = _lib()
    torch.manual_seed(S * 100 + nppf)
    td = t16(dtype)
    n_vid = S // nfrm
    n_lang = n_vid if lpv else 1            # nc_v = n_vid: every video shares language row 0 when lpv = 0
    nc_v = 1 if lpv else n_vid
    Nq = nsrl * nppf
    npad_q, npad_kv = (Nq + 31) // 32 * 32, (nppf + 31) // 32 * 32
    hd = H * dp
    qv = torch.zeros(S, H, nppf, dp, device="cuda"); kvv = torch.zeros_like(qv); vvv = torch.zeros_like(qv)
    qv[..., :dh] = torch.randn(S, H, nppf, dh, device="cuda")
    kvv[..., :dh] = torch.randn(S, H, nppf, dh, device="cuda")
    vvv[..., :dh] = torch.randn(S, H, nppf, dh, device="cuda")
    pl = torch.zeros(n_lang * nsrl, 3, H, dp, device="cuda")
    pl[..., :dh] = torch.randn(n_lang * nsrl, 3, H, dh, device="cuda")
    if spread != 1.0:
        # sharp attention: query and key parts scaled (values untouched) and put on a grid of 1/4 below 32, so that every
        # operand AND the sum Qv + Ql are exact in bf16 / f16: kernel and reference then see the same logits (up to fp32
        # summation order) and what is compared is the softmax arithmetic alone - the kernel rounds Qv and Ql separately,
        # which at 10 nats of logit spread would otherwise dominate the comparison (6 % on competing probabilities)
        grid = lambda t: (t * spread * 4).round().clamp(-60, 60) / 4
        qv, kvv = grid(qv) / 2, grid(kvv)
        pl[:, :2] = grid(pl[:, :2])
        pl[:, 0] /= 2
    lrow = torch.tensor([(s // nfrm) if lpv else (s // nfrm) // nc_v for s in range(S)], device="cuda")
    pls = pl.view(n_lang, nsrl, 3, H, dp)[lrow]                     # [S, nsrl, 3, H, dp]
    ql, kl, vl = (pls[:, :, i].permute(0, 2, 1, 3) for i in range(3))   # [S, H, nsrl, dp]
    # what the structured QKV epilogue stores: q fanned out (one rounding of the sum), k / v visual only
    if qvis:   # queries formed in the kernel from the 16-bit visual part + the fp32 language part
        q_tok = (qv.to(td).float().unsqueeze(2) + ql.unsqueeze(3)).reshape(S, H, Nq, dp).to(td)
    else:
        q_tok = (qv.unsqueeze(2) + ql.unsqueeze(3)).reshape(S, H, Nq, dp).to(td)
    kv16, vv16 = kvv.to(td), vvv.to(td)
    u_box = torch.randn(n_vid, nfrm * nppf, H, device="cuda") * 2
    peb = torch.randn(H, device="cuda")
    out = torch.full((S * Nq, hd), float("nan"), device="cuda").to(td)
    inv_scale = 1.0 / math.sqrt(H * dh)
    a = L.AttnStructArgs()
    qf, kf, vf = to_frag(qv.to(td) if qvis else q_tok, "qk"), to_frag(kv16, "qk"), to_frag(vv16, "v")
    a.q_visual = qvis
    plc = pl.reshape(n_lang * nsrl, 3 * hd).contiguous()
    a.q, a.kv, a.vv, a.pl, a.out16 = L.ptr(qf), L.ptr(kf), L.ptr(vf), L.ptr(plc), L.ptr(out)
    a.u, a.pe_b = L.ptr(u_box), L.ptr(peb)
    a.S, a.H, a.dp, a.nsrl, a.nppf, a.npad_q, a.npad_kv = S, H, dp, nsrl, nppf, npad_q, npad_kv
    a.nfrm, a.lang_per_vid, a.nc_v = nfrm, lpv, nc_v
    a.use_rel, a.seq_per_vid, a.NP, a.inv_scale, a.dtype = use_rel, nfrm, nfrm * nppf, inv_scale, DT[dtype]
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")      # (E x F form + its gated per-row fallback)
    a.guard_flag = L.ptr(guard)
    L.check(lib.vog_rel_attention_struct_fwd(C.byref(a), _sp()), "struct attention")
    torch.cuda.synchronize()
    raised = int(guard[0].item())
    # full reference over all (a', p') keys with the operands the kernel sees (16-bit rounded parts)
    klr, vlr = kl.to(td).float(), vl.to(td).float()
    k_tok = (kv16.float().unsqueeze(2) + klr.unsqueeze(3)).reshape(S, H, Nq, dp)
    v_tok = (vv16.float().unsqueeze(2) + vlr.unsqueeze(3)).reshape(S, H, Nq, dp)
    logits = q_tok.float() @ k_tok.transpose(-1, -2)
    if use_rel:
        ub = u_box.view(n_vid, nfrm, nppf, H)[torch.arange(S, device="cuda") // nfrm,
                                              torch.arange(S, device="cuda") % nfrm]        # [S, nppf, H]
        ut = ub.repeat(1, nsrl, 1).permute(0, 2, 1)                                         # [S, H, Nq]
        logits = logits + torch.relu(ut.unsqueeze(-1) - ut.unsqueeze(-2) + peb.view(1, -1, 1, 1))
    ref = torch.softmax(logits * inv_scale, dim=-1) @ v_tok
    got = out.float().view(S, Nq, H, dp).permute(0, 2, 1, 3)
    if spread != 1.0:
        xs = logits * inv_scale
        print(f"spread x{spread}: logit std {xs.std(-1).mean().item():.1f} nats, max - median "
              f"{(xs.max(-1).values - xs.median(-1).values).mean().item():.1f}; guard raised: {raised}")
        if spread >= 5.0:
            assert raised == 1, "rows 25+ nats under the shift must send the launch to the per-row kernel"
    else:
        assert raised == 0, "near-uniform attention must stay on the E x F kernel"
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    tol = (3e-2 if dtype == "bf16" else 5e-3) * max(1.0, ref.abs().max().item())
    assert err <= tol, (err, tol)


# ---- fused encoder tail (csrc/txtail.hip): Wo + residual + LN + FFN + residual + LN (+ lin2 + score) ----
def _pack32(w, dtype):
    """host fp32 [N, K] -> device tensor in the 32x16 fragment order of vog_pack_w_frag32."""
    w = np.ascontiguousarray(w.detach().cpu().numpy(), dtype=np.float32)
    N, K = w.shape
    dst = np.empty(N * K, dtype=np.uint16)
    L.check(_lib().vog_pack_w_frag32(w.ctypes.data, K, N, K, dst.ctypes.data, DT[dtype]), "pack32")
    return torch.from_numpy(dst.view(np.int16)).cuda()


def _ln(x, g, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,d,kwo,mode", [(800, 512, 576, "plain"), (1000, 768, 768, "vislang"),
                                          (1000, 768, 768, "score"), (77, 512, 576, "plain"),
                                          (4000, 768, 768, "score")])
def test_tx_tail_matches_torch_chain(M, d, kwo, mode, dtype):
    """One launch == the unfused chain with the same rounding points (attention output, x1, hidden and
    head operand rounded to 16 bit; everything else fp32). Tolerance: a 16-bit rounding flip of an
    operand element moves a 768-term fp32 dot product by ~1e-4 relative; LayerNorm outputs are O(1)."""
    torch.manual_seed(M + d)
    lib, T = _lib(), t16(dtype)
    dh = d // 2
    attn = (torch.randn(M, kwo, device="cuda") * 0.5).to(T)
    wo = torch.randn(d, kwo) / math.sqrt(kwo)
    w1 = torch.randn(dh, d) / math.sqrt(d)
    w2 = torch.randn(d, dh) / math.sqrt(dh)
    b1, b2 = torch.randn(dh, device="cuda") * 0.1, torch.randn(d, device="cuda") * 0.1
    g1, be1 = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    g2, be2 = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    a = L.TxTailArgs()
    keep = [attn, b1, b2, g1, be1, g2, be2]
    a.attn16, a.kwo = L.ptr(attn), kwo
    wo_p, w1_p, w2_p = _pack32(wo, dtype), _pack32(w1, dtype), _pack32(w2, dtype)
    a.wo_p, a.w1_p, a.w2_p = L.ptr(wo_p), L.ptr(w1_p), L.ptr(w2_p)
    a.ln1g, a.ln1b, a.b1, a.b2, a.ln2g, a.ln2b = (L.ptr(g1), L.ptr(be1), L.ptr(b1), L.ptr(b2), L.ptr(g2),
                                                  L.ptr(be2))
    if mode == "plain":
        res = torch.randn(M, d, device="cuda")
        a.residual, a.ldr = L.ptr(res), d
    else:
        # implicit vis||lang token rows: M = n_vid*nfrm*nsrl*nppf
        nfrm, nsrl, nppf = 10, 5, 20
        n_vid = M // (nfrm * nsrl * nppf)
        assert n_vid * nfrm * nsrl * nppf == M
        dv, dl = 512, 256
        vis = torch.randn(n_vid * nfrm * nppf, dv, device="cuda")
        lang = torch.randn(n_vid * nsrl, dl, device="cuda")
        va = L.VislangArgs()
        va.vis, va.lang = L.ptr(vis), L.ptr(lang)
        va.n_vid, va.nfrm, va.nppf, va.nsrl, va.dv, va.dl = n_vid, nfrm, nppf, nsrl, dv, dl
        va.lang_per_vid, va.nc_v, va.dtype = 0, 1, DT[dtype]
        a.res_vislang = C.addressof(va)
        v4 = vis.view(n_vid, nfrm, 1, nppf, dv).expand(-1, -1, nsrl, -1, -1)
        l4 = lang.view(n_vid, 1, nsrl, 1, dl).expand(-1, nfrm, -1, nppf, -1)
        res = torch.cat([v4, l4], -1).reshape(M, d)
    y32 = torch.full((M, d), float("nan"), device="cuda")
    y16 = torch.zeros(M, d, dtype=T, device="cuda")
    nscr = int(lib.vog_tx_tail_scratch_bytes(M, d))
    scr = torch.empty(max(nscr, 16), dtype=torch.uint8, device="cuda")
    a.x1_scratch = L.ptr(scr)
    a.M, a.d, a.dh, a.dtype = M, d, dh, DT[dtype]
    # torch reference, same rounding points
    wo_r, w1_r, w2_r = (w.cuda().to(T).float() for w in (wo, w1, w2))
    x1 = _ln(attn.float() @ wo_r.t() + res, g1, be1)
    hid = torch.relu(x1.to(T).float() @ w1_r.t() + b1).to(T).float()
    y = _ln(x1 + hid @ w2_r.t() + b2, g2, be2)
    if mode == "score":
        wl = torch.randn(256, d) / math.sqrt(d)
        bl = torch.randn(256, device="cuda") * 0.1
        wl2 = torch.randn(256, device="cuda") / 16
        bl2 = torch.randn(1, device="cuda")
        wl_p = _pack32(wl, "f16")
        arg_msk = torch.randint(0, 2, (n_vid, nsrl), device="cuda", dtype=torch.int64)
        cmp_msk = torch.randint(0, 2, (n_vid, 4), device="cuda", dtype=torch.int64)
        outs = torch.full((n_vid, 1, nsrl, nfrm * nppf), float("nan"), device="cuda")
        outs_eval = torch.full_like(outs, float("nan"))
        sa = L.ScoreArgs()
        sa.w2, sa.b2, sa.arg_msk, sa.cmp_msk = L.ptr(wl2), L.ptr(bl2), L.ptr(arg_msk), L.ptr(cmp_msk)
        sa.outs, sa.outs_eval = L.ptr(outs), L.ptr(outs_eval)
        sa.n_vid, sa.nfrm, sa.nppf, sa.nsrl, sa.dh = n_vid, nfrm, nppf, nsrl, 256
        sa.conc_type, sa.ncmp, sa.nc_v, sa.nvl, sa.nfrm0, sa.nppf0 = L.CONC_TYPE["spat"], 4, 1, 1, 10, 5
        a.wl_p, a.bl, a.score, a.head_dtype = L.ptr(wl_p), L.ptr(bl), C.addressof(sa), L.VOG_F16
    else:
        a.y32, a.y16 = L.ptr(y32), L.ptr(y16)
    L.check(lib.vog_tx_tail_fwd(C.byref(a), _sp()), "tx_tail")
    torch.cuda.synchronize()
    if mode != "score":
        err = (y32 - y).abs().max().item()
        print("tail y32 max abs err", err)
        assert err <= 4e-3, err
        assert (y16.float() - y).abs().max().item() <= 3e-2
        return
    h1 = torch.relu(y.half().float() @ wl.cuda().half().float().t() + bl)
    logit = (h1 @ wl2 + bl2).view(n_vid, nfrm, nsrl, nppf).permute(0, 2, 1, 3).reshape(n_vid, 1, nsrl, nfrm * nppf)
    err = (outs - logit).abs().max().item()
    print("tail logit max abs err", err)
    assert err <= 4e-3, err
    cmp = (torch.arange(nfrm * nppf, device="cuda") // 5) % 4
    ref_eval = torch.sigmoid(logit) * arg_msk.view(n_vid, 1, nsrl, 1).float() * cmp_msk[:, cmp].view(n_vid, 1, 1, -1).float()
    assert (outs_eval - ref_eval).abs().max().item() <= 1.5e-3
    assert torch.all(outs_eval[ref_eval == 0] == 0)


@pytest.mark.parametrize("lean", [0, 1])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("rows,nppf0", [(800, 5), (75, 5), (1600, 100), (8300, 100)])
def test_vis_encode_fused(rows, nppf0, dtype, lean):
    """Both feature encoders + the prop||seg concat in one launch, from the fp32 features, against
    relu(Linear) on the same 16-bit-rounded operands (mdl_vog.py:291-314, mdl_conc_single.py:51-66)."""
    torch.manual_seed(rows)
    lib, T = _lib(), t16(dtype)
    Kp, Ks, Np, Ns = 2048, 3072, 256, 256
    prop = torch.randn(rows, Kp, device="cuda")
    seg = torch.randn(rows // nppf0, Ks, device="cuda")
    wp, wsg = torch.randn(Np, Kp) / math.sqrt(Kp), torch.randn(Ns, Ks) / math.sqrt(Ks)
    bp, bs = torch.randn(Np, device="cuda") * 0.1, torch.randn(Ns, device="cuda") * 0.1

    def pack(w):
        w = np.ascontiguousarray(w.numpy(), dtype=np.float32)
        dst = np.empty(w.size, dtype=np.uint16)
        L.check(lib.vog_pack_w_frag(w.ctypes.data, w.shape[1], w.shape[0], w.shape[1], dst.ctypes.data, DT[dtype]), "pack")
        return torch.from_numpy(dst.view(np.int16)).cuda()

    wpf, wsf = pack(wp), pack(wsg)
    c32 = torch.full((rows, Np + Ns), float("nan"), device="cuda")
    c16 = torch.zeros(rows, Np + Ns, dtype=torch.bfloat16, device="cuda")
    a = L.VisencArgs()
    a.prop, a.seg, a.w_prop_f, a.w_seg_f, a.b_prop, a.b_seg = (L.ptr(prop), L.ptr(seg), L.ptr(wpf), L.ptr(wsf),
                                                                L.ptr(bp), L.ptr(bs))
    a.c32, a.c16, a.ldc, a.c16_dtype = L.ptr(c32), L.ptr(c16), Np + Ns, L.VOG_BF16
    a.n_prop_rows, a.nppf0, a.prop_dim, a.seg_dim, a.prop_enc, a.seg_enc, a.dtype = rows, nppf0, Kp, Ks, Np, Ns, DT[dtype]
    a.lean = lean
    assert lib.vog_vis_encode_supported(Kp, Ks, Np, Ns) == 1
    L.check(lib.vog_vis_encode(C.byref(a), _sp()), "vis_encode")
    torch.cuda.synchronize()
    rp = torch.relu(prop.to(T).float() @ wp.cuda().to(T).float().t() + bp)
    rs = torch.relu(seg.to(T).float() @ wsg.cuda().to(T).float().t() + bs).repeat_interleave(nppf0, dim=0)
    ref = torch.cat([rp, rs], 1)
    err = (c32 - ref).abs().max().item()
    assert err <= 2e-3, err
    assert (c16.float() - ref).abs().max().item() <= 3e-2


@pytest.mark.parametrize("S,N,H,d,use_rel", [(4, 200, 3, 512, 1), (6, 100, 3, 768, 1), (3, 67, 3, 512, 0)])
def test_encoder_layer_fwd_matches_plain_torch_layer(S, N, H, d, use_rel):
    """vog_encoder_layer_fwd (one call = QKV projection -> RelAttention -> Wo/LN/FFN/LN tail) against a
    plain fp32 torch (Rel)EncoderLayer on the same 16-bit-rounded operands (transformer_code.py:128-203:
    torch.chunk heads, scale sqrt(d_model), bias relu(u_i - u_j + b_h) added before the scaling)."""
    lib = _lib()
    torch.manual_seed(S * 7 + N)
    dtype, T = "bf16", torch.bfloat16
    heads = vo.chunk_sizes(d, H)
    dp = (max(heads) + 31) // 32 * 32
    npad = (N + 31) // 32 * 32
    dh = d // 2
    M = S * N
    x = torch.randn(M, d, device="cuda")
    x16 = x.to(T)
    wq, wk, wv = (torch.randn(d, d) / math.sqrt(d) for _ in range(3))
    wo = torch.randn(d, d) / math.sqrt(d)
    w1 = torch.randn(dh, d) / math.sqrt(d)
    w2 = torch.randn(d, dh) / math.sqrt(dh)
    b1, b2 = torch.randn(dh, device="cuda") * 0.1, torch.randn(d, device="cuda") * 0.1
    g1, be1 = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    g2, be2 = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    # padded weights (heads padded to dp with zero rows / columns)
    wqkv_pad = torch.zeros(3 * H * dp, d)
    wo_pad = torch.zeros(d, H * dp)
    off = 0
    for h, hd_ in enumerate(heads):
        for which, w in enumerate((wq, wk, wv)):
            wqkv_pad[(which * H + h) * dp:(which * H + h) * dp + hd_] = w[off:off + hd_]
        wo_pad[:, h * dp:h * dp + hd_] = wo[:, off:off + hd_]
        off += hd_
    wqkv16 = wqkv_pad.cuda().to(T)
    u_box = torch.randn(S, N, H, device="cuda") * 2
    peb = torch.randn(H, device="cuda")
    q = torch.zeros(S, H, npad * dp, device="cuda").to(T)
    k, vt = torch.zeros_like(q), torch.zeros_like(q)
    attn16 = torch.zeros(M, H * dp, device="cuda").to(T)
    y32 = torch.full((M, d), float("nan"), device="cuda")
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    wo_p, w1_p, w2_p = _pack32(wo_pad, dtype), _pack32(w1, dtype), _pack32(w2, dtype)
    a = L.EncoderLayerArgs()
    a.qkv.x16, a.qkv.ldx, a.qkv.wqkv, a.qkv.ldw = L.ptr(x16), d, L.ptr(wqkv16), d
    a.qkv.q, a.qkv.k, a.qkv.vt = L.ptr(q), L.ptr(k), L.ptr(vt)
    a.qkv.S, a.qkv.N, a.qkv.H, a.qkv.dp, a.qkv.npad, a.qkv.K, a.qkv.dtype = S, N, H, dp, npad, d, DT[dtype]
    a.attn.q, a.attn.k, a.attn.vt, a.attn.out16 = L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(attn16)
    a.attn.u, a.attn.pe_b = L.ptr(u_box), L.ptr(peb)
    a.attn.S, a.attn.N, a.attn.H, a.attn.dp, a.attn.npad = S, N, H, dp, npad
    a.attn.use_rel, a.attn.n_box, a.attn.seq_per_vid, a.attn.NP = use_rel, N, 1, N
    a.attn.inv_scale, a.attn.dtype, a.attn.guard_flag = 1.0 / math.sqrt(d), DT[dtype], L.ptr(flag)
    a.tail.attn16, a.tail.kwo = L.ptr(attn16), H * dp
    a.tail.wo_p, a.tail.w1_p, a.tail.w2_p = L.ptr(wo_p), L.ptr(w1_p), L.ptr(w2_p)
    a.tail.residual, a.tail.ldr = L.ptr(x), d
    a.tail.ln1g, a.tail.ln1b, a.tail.b1, a.tail.b2, a.tail.ln2g, a.tail.ln2b = (
        L.ptr(g1), L.ptr(be1), L.ptr(b1), L.ptr(b2), L.ptr(g2), L.ptr(be2))
    a.tail.y32, a.tail.y16_dtype, a.tail.head_dtype = L.ptr(y32), -1, L.VOG_F16
    a.tail.M, a.tail.d, a.tail.dh, a.tail.dtype = M, d, dh, DT[dtype]
    L.check(lib.vog_encoder_layer_fwd(C.byref(a), _sp()), "encoder layer")
    torch.cuda.synchronize()
    # plain torch layer on the operands the kernels see
    r16 = lambda w: w.cuda().to(T).float()                                    # noqa: E731
    xs = x16.float().view(S, N, d)
    qh = (xs @ r16(wq).t()).to(T).float()
    kh = (xs @ r16(wk).t()).to(T).float()
    vh = (xs @ r16(wv).t()).to(T).float()
    outs, off = [], 0
    for h, hd_ in enumerate(heads):
        logits = qh[..., off:off + hd_] @ kh[..., off:off + hd_].transpose(-1, -2)
        if use_rel:
            uh = u_box[..., h]
            logits = logits + torch.relu(uh.unsqueeze(-1) - uh.unsqueeze(-2) + peb[h])
        pa = torch.softmax(logits / math.sqrt(d), dim=-1)
        outs.append(pa @ vh[..., off:off + hd_])
        off += hd_
    att = torch.cat(outs, -1).reshape(M, d).to(T).float()
    x1 = _ln(att @ r16(wo).t() + x, g1, be1)
    hid = torch.relu(x1.to(T).float() @ r16(w1).t() + b1).to(T).float()
    y = _ln(x1 + hid @ r16(w2).t() + b2, g2, be2)
    err = (y32 - y).abs().max().item()
    print("encoder layer max abs err", err)
    assert torch.isfinite(y32).all()
    assert err <= 2.5e-2, err                       # P is rounded to bf16 inside the attention (LayerNorm outputs are O(1))
    assert (y32 - y).abs().mean().item() <= 1.5e-3
    # inconsistent argument blocks are refused
    a.tail.M = M - 1
    assert lib.vog_encoder_layer_fwd(C.byref(a), _sp()) != 0
