"""-m gpu: the language chain behind the BiLSTM and the prediction head through the C ABI - the argument-vector kernel in its
one-round and two-round forms, the out-projection shapes of the M <= 64 GEMM (alone and as one half of a pair launch), and the
few-proposal form of the prediction head."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import vog_oracle as vo
from tests.gpu_util import L, build_engine

pytestmark = pytest.mark.gpu


def _sp():
    return L.stream_ptr()


# ---- vog_srl_argvec -------------------------------------------------------------------------------------------------------
AV_ROWS, AV_STAGE_FLOATS = 20, 256 * 16 * 4


def _one_round(Bn, T, nsrl, Ld):
    """The rule of the host wrapper (csrc/elementwise.hip, vog_srl_argvec): the sentences that the widest group of 20 rows
    touches, T rows of Ld floats each, fit 64 KiB."""
    rows = Bn * nsrl
    nb = max((min(r0 + AV_ROWS, rows) - 1) // nsrl - r0 // nsrl + 1 for r0 in range(0, rows, AV_ROWS))
    return nb * T * Ld <= AV_STAGE_FLOATS


def _argvec_inputs(Bn, T, nsrl, Ld, seed):
    g = np.random.default_rng(seed)
    full = g.standard_normal((Bn * T, Ld)).astype(np.float32)
    cap = g.integers(-2, T + 2, size=(Bn * nsrl, 2)).astype(np.int64)       # below 0 and at / above T: the clamps
    msk = g.integers(0, 2, size=(Bn * nsrl,)).astype(np.int64)
    msk[0] = 1
    if msk.size > 1:
        msk[-1] = 0
    w = (g.standard_normal((Ld, 2 * Ld)) / math.sqrt(2 * Ld)).astype(np.float32)
    bias = g.standard_normal((Ld,)).astype(np.float32)
    return full, cap, msk, w, bias


def _argvec_gpu(full, cap, msk, w, bias, Bn, T, nsrl, Ld):
    lib = L.load()
    d = [torch.from_numpy(x).cuda() for x in (full, cap, msk, w, bias)]
    lang = torch.full((Bn * nsrl, Ld), float("nan"), device="cuda")
    L.check(lib.vog_srl_argvec(*[L.ptr(x) for x in d], L.ptr(lang), Bn, T, nsrl, Ld, _sp()), "argvec")
    torch.cuda.synchronize()
    return lang.cpu()


def _argvec_ref(full, cap, msk, w, bias, Bn, T, nsrl):
    """float64; returns (value, sum |w||x|) per output."""
    c = np.clip(cap, 0, T - 1)
    b = np.arange(Bn * nsrl) // nsrl
    x = np.concatenate([full[b * T + c[:, 0]], full[b * T + c[:, 1]]], axis=1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = x @ w.astype(np.float64).T + bias.astype(np.float64)
        v = np.where(v < 0, 0.0, v) * msk[:, None]
        mag = np.abs(x) @ np.abs(w.astype(np.float64)).T
    return v, mag


@pytest.mark.parametrize("T", [1, 12])
@pytest.mark.parametrize("Ld", [256, 64])
@pytest.mark.parametrize("Bn,nsrl", [(1, 1), (1, 5), (4, 5), (3, 7), (7, 3), (21, 1)])
def test_argvec_against_float64(Bn, nsrl, Ld, T):
    """1, 5, 20 and 21 rows (21: a second row group, aligned and not aligned to a sentence); Ld = 256 (compile-time slices) and
    64 (general path). (7, 3) and (21, 1) at T = 12, Ld = 256 exceed the one-round staging: the two-round form."""
    inp = _argvec_inputs(Bn, T, nsrl, Ld, seed=Bn * 100 + nsrl * 10 + T)
    got = _argvec_gpu(*inp, Bn, T, nsrl, Ld).numpy().astype(np.float64)
    ref, mag = _argvec_ref(*inp, Bn, T, nsrl)
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= 1e-5 * mag).all(), float((np.abs(got - ref) / mag).max())
    assert (got[inp[2] == 0] == 0.0).all()


def test_argvec_form_rule_covers_both_forms():
    assert _one_round(4, 12, 5, 256) and _one_round(3, 12, 7, 256) and _one_round(21, 1, 1, 256)
    assert not _one_round(7, 12, 3, 256) and not _one_round(21, 12, 1, 256) and not _one_round(20, 30, 1, 64)


@pytest.mark.parametrize("Ld,T", [(256, 12), (64, 30)])
def test_argvec_one_round_equals_two_round(Ld, T):
    """The same 20 dot products as 4 sentences x 5 arguments (staged whole: one round) and as 20 sentences x 1 argument (too
    many rows to stage: two rounds): same slices, same order -> the same bits."""
    Bn, nsrl = 4, 5
    full, cap, msk, w, bias = _argvec_inputs(Bn, T, nsrl, Ld, seed=7)
    assert _one_round(Bn, T, nsrl, Ld) and not _one_round(Bn * nsrl, T, 1, Ld)
    a = _argvec_gpu(full, cap, msk, w, bias, Bn, T, nsrl, Ld)
    full20 = np.ascontiguousarray(full.reshape(Bn, 1, T, Ld).repeat(nsrl, axis=1).reshape(Bn * nsrl * T, Ld))
    b = _argvec_gpu(full20, cap, msk, w, bias, Bn * nsrl, T, 1, Ld)
    assert torch.equal(a, b)


@pytest.mark.parametrize("Bn,nsrl", [(4, 5), (21, 1)])
def test_argvec_nan_row_reaches_the_output(Bn, nsrl):
    """A poisoned row of `full` (the persistent BiLSTM's hand-off time-out) comes out as NaN (relu_nan) in exactly the rows that
    select it - in both forms."""
    T, Ld = 12, 256
    full, cap, msk, w, bias = _argvec_inputs(Bn, T, nsrl, Ld, seed=11)
    msk[:] = 1
    cap = np.clip(cap, 0, T - 1)
    cap[0] = (3, 5)
    full[0 * T + 5] = np.nan
    got = _argvec_gpu(full, cap, msk, w, bias, Bn, T, nsrl, Ld).numpy()
    hit = ((np.arange(Bn * nsrl) // nsrl == 0) & ((cap[:, 0] == 5) | (cap[:, 1] == 5)))
    assert hit[0] and np.isnan(got[hit]).all() and np.isfinite(got[~hit]).all()


# ---- out-projection -------------------------------------------------------------------------------------------------------
def _frag_a(a):
    M, K = a.shape
    m = torch.arange(M, device=a.device).view(-1, 1)
    k = torch.arange(K, device=a.device).view(1, -1)
    idx = ((((m >> 4) * (K >> 5) + (k >> 5)) * 64) + (((k >> 3) & 3) << 4) + (m & 15)) * 8 + (k & 7)
    af = torch.zeros((M + 15) // 16 * 16 * K, dtype=a.dtype, device=a.device)
    af[idx.reshape(-1)] = a.reshape(-1)
    return af


@pytest.mark.parametrize("a_frag", [0, 1])
@pytest.mark.parametrize("K", [2048, 128])
@pytest.mark.parametrize("M", [5, 52, 64])
def test_outproj_gemm_shapes(M, K, a_frag):
    """[out16 ; h_final] x W_outproj^T + bias, ReLU: 256 columns, fragment-ordered weights, plain and fragment-ordered A."""
    lib = L.load()
    N = 256
    torch.manual_seed(M + K + a_frag)
    a = torch.randn(M, K, device="cuda").half()
    w = (torch.randn(N, K) / math.sqrt(K)).contiguous()
    wf = np.zeros(N * K, np.uint16)
    L.check(lib.vog_pack_w_frag(w.numpy().ctypes.data, K, N, K, wf.ctypes.data, L.VOG_F16), "pack")
    wfd = torch.from_numpy(wf.view(np.int16)).cuda()
    bias = torch.randn(N, device="cuda")
    ad = _frag_a(a) if a_frag else a
    g = L.GemmArgs()
    g.a, g.a_is_f32, g.lda, g.w, g.ldw, g.w_frag, g.a_frag = L.ptr(ad), 0, K, L.ptr(wfd), K, 1, a_frag
    c32 = torch.full((M, N), float("nan"), device="cuda")
    g.bias, g.c32, g.ldc, g.M, g.N, g.K, g.relu, g.rep, g.dtype = L.ptr(bias), L.ptr(c32), N, M, N, K, 1, 1, L.VOG_F16
    L.check(lib.vog_gemm_bias_act(C.byref(g), _sp()), "gemm")
    torch.cuda.synchronize()
    ref = torch.relu(a.float() @ w.cuda().half().float().t() + bias)
    assert (c32 - ref).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("name", ["small/vog_spat", "full/cfg2_vog_spat_gt5_bs4"])
def test_paired_outproj_equals_separate_launches(name):
    """The out-projection shares its launch with mul_tx's QKV projection through the one-row-tile body of csrc/gemm_dev.h; alone
    it is the general M <= 64 kernel. Same k order per wave, same order of the waves' partial sums -> bit-identical outputs."""
    eng, cfg, sd, batch, c, dev = build_engine(name, cached=True)
    eng.set_option("enc_lean", 1)            # (the encoder form otherwise follows the pairing decision)
    eng.set_option("pair_launches", 0)
    a = {k: v.clone() for k, v in eng.forward(dev).items() if isinstance(v, torch.Tensor)}
    eng.set_option("pair_launches", 1)
    b = eng.forward(dev)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), (name, k)


# ---- prediction head ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conc", ["spat", "temp", "sep"])
@pytest.mark.parametrize("np0,ncmp", [(1, 4), (5, 4), (7, 4), (7, 2), (5, 5), (9, 4)])
def test_pred_head_few_proposals_exact(conc, np0, ncmp):
    """1, 5 and 7 proposals per frame with at most 4 videos: boxes requested with the scores; (5, 5) and (9, 4): the general
    form. Records byte-equal to the oracle head: ties (first index wins) and all-zero (masked) scores included."""
    lib = L.load()
    torch.manual_seed(np0 * 10 + ncmp)
    B, nsrl, nf = 3, 5, 10
    oc = vo.OracleCfg(conc_type=conc, nppf0=np0)
    if conc == "sep":
        ev = torch.rand(B, ncmp, nsrl, nf * np0)
        props = torch.rand(B, ncmp, nf * np0, 7)
    else:
        ev = torch.rand(B, 1, nsrl, ncmp * nf * np0)
        props = torch.rand(B, ncmp * nf * np0, 7)
    ev[0, 0, 4] = 0.0                         # masked argument: all ties -> first index
    ev[1, 0, 1, : np0 + 2] = 0.5              # exact ties: a whole frame and the start of the next
    ev[2, 0, 2, np0 - 1] = 2.0                # the maximum in the last proposal of a frame ...
    ev[2, 0, 2, 2 * np0 - 1] = 2.0            # ... and the same value again in the next frame / video
    ev[2, 0, 3, : 2 * np0] = 0.25
    ev[2, 0, 3, np0 // 2] = 0.75              # the maximum twice inside one frame (np0 >= 5)
    ev[2, 0, 3, np0 - 1] = 0.75
    fin = torch.rand(B, ncmp)
    fin[1, :] = 0.5                           # tie over the videos
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
