"""-m gpu: the hi + lo operand kernels at the long-sequence shapes (100 proposals per frame; gt5 spat with 6 or more videos per
query): plain attention over more than 256 tokens, separable mul_tx layer-0 attention over several visual key blocks, the feature
encoders with the segment replicas copied by vog_seg_replicate. Operands, fp32 references on the UNROUNDED operands, tolerances
and assertions are those of tests/test_gpu_split.py (2.5e-3 / 3e-3 of the value scale, the plain f16 kernel on the same data more
than 3 x worse, out16 + out16_lo, the logit report)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.gpu_util import L
from tests.test_gpu_ops import DT, _attn_ref, _lib, _sp, to_frag
from tests import test_gpu_split as _ts
from tests.test_gpu_split import _pack16, hi_lo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S,N,H,dh,dp,nsrl,use_rel", [
    (4, 300, 3, 171, 192, 1, 1), (2, 480, 3, 171, 192, 1, 1), (2, 1000, 3, 171, 192, 1, 1), (4, 4000, 3, 171, 192, 1, 1),
    (3, 2000, 3, 256, 256, 5, 1), (2, 1030, 2, 64, 64, 1, 0)])
def test_rel_attention_hi_lo_long(S, N, H, dh, dp, nsrl, use_rel):
    """tests/test_gpu_split.py::test_rel_attention_hi_lo at more than 256 tokens (the running-maximum tile kernel with the K
    remainders in its LDS ring): same operands, reference, tolerances and assertions."""
    lib = _lib()
    torch.manual_seed(S * 1000 + N)
    npad = (N + 31) // 32 * 32
    q = torch.zeros(S, H, N, dp, device="cuda"); k = torch.zeros_like(q); v = torch.zeros_like(q)
    sc = math.sqrt(20.0 * math.sqrt(H * dh) / math.sqrt(dh))          # logits / sqrt(H dh) with std ~ 20
    q[..., :dh] = torch.randn(S, H, N, dh, device="cuda") * sc
    k[..., :dh] = torch.randn(S, H, N, dh, device="cuda") * sc
    v[..., :dh] = torch.randn(S, H, N, dh, device="cuda")
    (qh, ql), (kh, kl) = hi_lo(q), hi_lo(k)
    v16 = v.to(torch.float16)
    n_box = N // nsrl
    u_box = torch.randn(S, n_box, H, device="cuda") * 3
    peb = torch.randn(H, device="cuda")
    inv_scale = 1.0 / math.sqrt(H * dh)
    u_tok = u_box.repeat(1, nsrl, 1)
    ref = _attn_ref(q, k, v16.float(), u_tok, peb, n_box, inv_scale, use_rel)      # fp32 q, k
    outs = {}
    for split in (0, 1):
        out = torch.full((S * N, H * dp), float("nan"), device="cuda").to(torch.float16)
        out_lo = torch.full_like(out, float("nan"))
        lmax = torch.zeros(L.LOGIT_WORDS * L.LOGIT_STRIDE, dtype=torch.int32, device="cuda")   # (vog_attn_args.logit_max: 4 KiB)
        a = L.AttnArgs()
        frs = [to_frag(qh, "qk"), to_frag(kh, "qk"), to_frag(v16, "v")]       # (kept alive: the kernel reads them)
        a.q, a.k, a.vt, a.out16 = L.ptr(frs[0]), L.ptr(frs[1]), L.ptr(frs[2]), L.ptr(out)
        a.u, a.pe_b = L.ptr(u_box.contiguous()), L.ptr(peb)
        a.S, a.N, a.H, a.dp, a.npad = S, N, H, dp, npad
        a.use_rel, a.n_box, a.seq_per_vid, a.NP = use_rel, n_box, 1, n_box
        a.inv_scale, a.dtype = inv_scale, DT["f16"]
        a.logit_max = L.ptr(lmax)
        keep = []
        if split:
            keep = [to_frag(ql, "qk"), to_frag(kl, "qk")]
            a.q_lo, a.k_lo, a.out16_lo = L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(out_lo)
        L.check(lib.vog_rel_attention_fwd(C.byref(a), _sp()), "attn")
        torch.cuda.synchronize()
        got = out.float().view(S, N, H, dp).permute(0, 2, 1, 3)
        assert torch.isfinite(got).all()
        outs[split] = (got - ref).abs().max().item()
        if split:
            full = (out.float() + out_lo.float()).view(S, N, H, dp).permute(0, 2, 1, 3)
            e2 = (full - ref).abs().max().item()
            # P and V are still f16 (2^-11 each, averaged by the sum): 2e-3 of the value scale
            assert e2 <= 2e-3 * max(1.0, ref.abs().max().item()), e2
            assert (full[..., dh:] == 0).all()
        lg = (q @ k.transpose(-1, -2))
        if use_rel:
            ub = u_tok.permute(0, 2, 1)
            lg = lg + torch.relu(ub.unsqueeze(-1) - ub.unsqueeze(-2) + peb.view(1, -1, 1, 1))
        want = (lg * inv_scale).abs().max().item()
        seen = float(lmax.cpu().numpy().view(np.float32).max())
        if split:                             # (the plain long-sequence kernels do not report)
            assert abs(seen - want) <= 1e-3 * want, (seen, want)
    print(f"max abs error vs fp32 logits: plain f16 {outs[0]:.2e}, hi + lo {outs[1]:.2e}")
    assert outs[1] <= 2.5e-3 * max(1.0, ref.abs().max().item())
    assert outs[0] > 3 * outs[1]            # the case is sharp enough to tell the two apart


@pytest.mark.parametrize("S,nfrm,nsrl,nppf,H,dh,dp,use_rel,lpv", [
    (20, 10, 5, 40, 3, 256, 256, 1, 0), (20, 10, 5, 100, 3, 256, 256, 1, 1), (10, 10, 5, 400, 3, 256, 256, 1, 0),
    (20, 10, 5, 100, 3, 128, 128, 1, 0)])
def test_rel_attention_struct_hi_lo_blocks(S, nfrm, nsrl, nppf, H, dh, dp, use_rel, lpv):
    """tests/test_gpu_split.py::test_rel_attention_struct_hi_lo over several visual key blocks (the LDS-ring kernel with the K
    remainders in a ring of two slots): same operands, reference, tolerances and assertions."""
    lib = _lib()
    torch.manual_seed(S * 100 + nppf)
    n_vid = S // nfrm
    n_lang = n_vid if lpv else 1
    nc_v = 1 if lpv else n_vid
    Nq, hd = nsrl * nppf, H * dp
    npad_kv = (nppf + 31) // 32 * 32
    sc = math.sqrt(20.0 * math.sqrt(H * dh) / math.sqrt(dh) / 2.0)
    qv = torch.zeros(S, H, nppf, dp, device="cuda"); kvv = torch.zeros_like(qv); vvv = torch.zeros_like(qv)
    qv[..., :dh] = torch.randn(S, H, nppf, dh, device="cuda") * sc
    kvv[..., :dh] = torch.randn(S, H, nppf, dh, device="cuda") * sc
    vvv[..., :dh] = torch.randn(S, H, nppf, dh, device="cuda")
    pl = torch.zeros(n_lang * nsrl, 3, H, dp, device="cuda")
    pl[..., :dh] = torch.randn(n_lang * nsrl, 3, H, dh, device="cuda")
    pl[:, :2] *= sc
    lrow = torch.tensor([(s // nfrm) if lpv else (s // nfrm) // nc_v for s in range(S)], device="cuda")
    pls = pl.view(n_lang, nsrl, 3, H, dp)[lrow]
    ql, kl, vl = (pls[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    (qh, qlo), (kh, klo) = hi_lo(qv), hi_lo(kvv)
    vv16 = vvv.to(torch.float16)
    u_box = torch.randn(n_vid, nfrm * nppf, H, device="cuda") * 2
    peb = torch.randn(H, device="cuda")
    inv_scale = 1.0 / math.sqrt(H * dh)
    plc = pl.reshape(n_lang * nsrl, 3 * hd).contiguous()
    # full fp32 reference (values as the kernel sees them: f16)
    q_tok = (qv.unsqueeze(2) + ql.unsqueeze(3)).reshape(S, H, Nq, dp)
    k_tok = (kvv.unsqueeze(2) + kl.unsqueeze(3)).reshape(S, H, Nq, dp)
    v_tok = (vv16.float().unsqueeze(2) + vl.to(torch.float16).float().unsqueeze(3)).reshape(S, H, Nq, dp)
    logits = q_tok @ k_tok.transpose(-1, -2)
    if use_rel:
        ub = u_box.view(n_vid, nfrm, nppf, H)[torch.arange(S, device="cuda") // nfrm, torch.arange(S, device="cuda") % nfrm]
        ut = ub.repeat(1, nsrl, 1).permute(0, 2, 1)
        logits = logits + torch.relu(ut.unsqueeze(-1) - ut.unsqueeze(-2) + peb.view(1, -1, 1, 1))
    ref = torch.softmax(logits * inv_scale, dim=-1) @ v_tok
    errs = {}
    for split in (0, 1):
        out = torch.full((S * Nq, hd), float("nan"), device="cuda").to(torch.float16)
        out_lo = torch.full_like(out, float("nan"))
        lmax = torch.zeros(L.LOGIT_WORDS * L.LOGIT_STRIDE, dtype=torch.int32, device="cuda")   # (vog_attn_args.logit_max: 4 KiB)
        a = L.AttnStructArgs()
        keep = [to_frag(qh, "qk"), to_frag(kh, "qk"), to_frag(vv16, "v"), to_frag(qlo, "qk"), to_frag(klo, "qk")]
        a.q_visual = 1
        a.q, a.kv, a.vv, a.pl, a.out16 = L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(plc), L.ptr(out)
        a.u, a.pe_b = L.ptr(u_box), L.ptr(peb)
        a.S, a.H, a.dp, a.nsrl, a.nppf, a.npad_q, a.npad_kv = S, H, dp, nsrl, nppf, (Nq + 31) // 32 * 32, npad_kv
        a.nfrm, a.lang_per_vid, a.nc_v = nfrm, lpv, nc_v
        a.use_rel, a.seq_per_vid, a.NP, a.inv_scale, a.dtype = use_rel, nfrm, nfrm * nppf, inv_scale, DT["f16"]
        a.logit_max = L.ptr(lmax)
        if split:
            a.q_lo, a.kv_lo, a.out16_lo = L.ptr(keep[3]), L.ptr(keep[4]), L.ptr(out_lo)
        L.check(lib.vog_rel_attention_struct_fwd(C.byref(a), _sp()), "struct attention")
        torch.cuda.synchronize()
        got = out.float().view(S, Nq, H, dp).permute(0, 2, 1, 3)
        assert torch.isfinite(got).all()
        errs[split] = (got - ref).abs().max().item()
        if split:
            # out16_lo = t16(o - t16(o)) of the fp32 result o: at most half an f16 ulp of out16 (2^-11 relative, 2^-25 near zero),
            # and out16 + out16_lo is o to ~2^-21 - inside the bound the 16-bit rows alone are held to
            lo = out_lo.float()
            assert torch.isfinite(lo).all()
            assert (lo.abs() <= out.float().abs() * 2.0 ** -11 + 2.0 ** -24).all()
            full = (out.float() + lo).view(S, Nq, H, dp).permute(0, 2, 1, 3)
            assert (full - ref).abs().max().item() <= 3e-3 * max(1.0, ref.abs().max().item())
            assert (full[..., dh:] == 0).all()
        seen = float(lmax.cpu().numpy().view(np.float32).max())
        want = (logits * inv_scale).abs().max().item()
        if split:                             # (the plain LDS-ring kernel does not report)
            assert want * 0.98 <= seen <= 2.05 * want, (seen, want)     # (a bound: max|x| + max|y| of the separable parts)
    print(f"struct attention, max abs error vs fp32: plain f16 {errs[0]:.2e}, hi + lo {errs[1]:.2e}")
    assert errs[1] <= 3e-3 * max(1.0, ref.abs().max().item())
    assert errs[0] > 3 * errs[1]


def test_vis_encode_hi_lo_p100():
    """100 proposals per frame, 16 000 rows, one call: the encoder launch writes replica 0 of every segment row and its own copy
    launch the other 99 (tests/test_gpu_split.py::test_vis_encode_hi_lo, unchanged)."""
    _ts.test_vis_encode_hi_lo(16000, 100)


def test_vis_encode_hi_lo_deferred_replicas():
    """vog_vis_encode with defer_replicas + vog_seg_replicate (the forward's two steps) with hi + lo operands at nppf0 = 100,
    16 000 rows, against the fp64 product as test_vis_encode_hi_lo: c32 to fp32 accuracy, c16 + c16_lo = c32 in EVERY replica."""
    lib = _lib()
    rows, nppf0 = 16000, 100
    torch.manual_seed(rows)
    Kp, Ks, Np, Ns = 2048, 3072, 256, 256
    prop = torch.randn(rows, Kp, device="cuda")
    seg = torch.randn(rows // nppf0, Ks, device="cuda")
    wp = torch.randn(Np, Kp, device="cuda") / math.sqrt(Kp)
    wsg = torch.randn(Ns, Ks, device="cuda") / math.sqrt(Ks)
    bp, bs = torch.randn(Np, device="cuda") * 0.1, torch.randn(Ns, device="cuda") * 0.1
    wph, wsh = wp.to(torch.float16).float(), wsg.to(torch.float16).float()
    keep = [_pack16(wph), _pack16(wsh), _pack16(wp - wph), _pack16(wsg - wsh)]
    ref = torch.cat([torch.relu(prop.double() @ wp.double().t() + bp.double()),
                     torch.relu(seg.double() @ wsg.double().t() + bs.double()).repeat_interleave(nppf0, 0)], 1).float()
    errs = {}
    for split in (0, 1):
        c32 = torch.full((rows, Np + Ns), float("nan"), device="cuda")
        c16 = torch.zeros(rows, Np + Ns, device="cuda").to(torch.float16)
        c16l = torch.full_like(c16, float("nan"))
        a = L.VisencArgs()
        a.prop, a.seg, a.w_prop_f, a.w_seg_f, a.b_prop, a.b_seg = L.ptr(prop), L.ptr(seg), L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(bp), L.ptr(bs)
        a.c32, a.c16, a.ldc, a.c16_dtype = L.ptr(c32), L.ptr(c16), Np + Ns, DT["f16"]
        a.n_prop_rows, a.nppf0, a.prop_dim, a.seg_dim, a.prop_enc, a.seg_enc, a.dtype, a.lean = rows, nppf0, Kp, Ks, Np, Ns, DT["f16"], 1
        a.defer_replicas = 1
        if split:
            a.w_prop_f_lo, a.w_seg_f_lo, a.c16_lo = L.ptr(keep[2]), L.ptr(keep[3]), L.ptr(c16l)
        L.check(lib.vog_vis_encode(C.byref(a), _sp()), "vis_encode")
        torch.cuda.synchronize()
        assert torch.isnan(c32[1, Np:]).all()                    # (replica 1 of the segment columns: not written yet)
        L.check(lib.vog_seg_replicate(C.byref(a), _sp()), "seg_replicate")
        torch.cuda.synchronize()
        errs[split] = (c32 - ref).abs().max().item()
        if split:
            assert (c16.float() + c16l.float() - c32).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())
    print(f"encoders at nppf0 = 100, max abs error vs fp64: plain f16 {errs[0]:.2e}, hi + lo {errs[1]:.2e}")
    assert errs[1] <= 5e-6 * max(1.0, ref.abs().max().item())
    assert errs[0] > 20 * errs[1]
