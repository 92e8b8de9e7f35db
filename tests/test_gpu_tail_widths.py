"""-m gpu: the fused encoder-layer tail at d = 256 and d = 384 (csrc/txtail.hip, TxTailBody<..., NW>): the widths that
`vsrl.prop / seg / lang_encode_size = 128` gives obj_tx and mul_tx.

  1. the operator against the torch chain with the same rounding points, bounds of tests/test_gpu_ops.py::
     test_tx_tail_matches_torch_chain (4e-3 on y32, 3e-2 on y16, 4e-3 on the logit, 1.5e-3 on outs_eval). Shapes: a partial row
     block (M = 77, 200), every kwo of each width's rule, and M = 4112 (65 row blocks: all eight k-step rotations,
     xpos = (block >> 3) & 7; f16, see ROT_CASES). The median row is at 1e-6; what the bound on the maximum sees is rows with a
     flipped 16-bit rounding of an x1 / hidden element (1 - 4 of 200 rows in bf16; seeded with M + d + kwo instead of that test's
     M + d, the (200, 384, 384, plain, bf16) case measured 4.2e-3 on one such row - the bound has no margin for bf16 flips here);
  2. probe and entry agree; remainder pointers are refused at the new widths; the obj pair launch equals two launches;
  3. - 7. the `w128` model (a model of those sizes, built here from synth like oracle/cases.build): launch trace, whole forward
     against the CPU oracle with fused_tail = 0 as the control, captured slot, plan gate, weight refresh, ObjBank rows.
At spat obj_tx has 400 rows (6 row blocks + 16 rows), mul_tx 2000 (31 + 16 rows: four rotation bands)."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import cases
from tests.gpu_util import L, comm_for, engine_mod, flat, objed, oracle_run, t16, trace
from tests.test_gpu_forward import _OracleGolden, _check_against
from tests.test_gpu_ops import DT, _ln, _pack32

pytestmark = pytest.mark.gpu
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
synth = importlib.import_module("vognet-pytorch_amd.synth")

W128 = {"mdl.prop_feat_dim": 256, "mdl.seg_feat_dim": 256, "mdl.input_encoding_size": 64, "mdl.rnn.rnn_size": 128,
        "mdl.vsrl.prop_encode_size": 128, "mdl.vsrl.seg_encode_size": 128, "mdl.vsrl.lang_encode_size": 128}
VOCAB, NPPF0, B, NCMP = 50, 5, 2, 4
MODELS = [("vog", "spat"), ("vog", "sep"), ("vog", "temp"), ("vgrnd", "spat")]
OUT_KEYS = ("mdl_outs", "mdl_outs_eval", "pred_rec")
UNFUSED = ("wo", "ln1", "ffn1", "ffn2", "ln2")
_BUILT = {}


def w128(mdl, conc):
    """-> (engine with every option at its default, cfg, sd, batch, c, oracle result), once per session"""
    key = (mdl, conc)
    if key not in _BUILT:
        cfg = ec.get_default_cfg()
        ec.update_from_dict(cfg, {"mdl.name": mdl, "ds.conc_type": conc, **cases.REL, **W128})
        c = {"vocab": VOCAB, "nppf0": NPPF0}
        sd = synth.init_state_dict(cfg, VOCAB, seed=1, perturb_ln=True)
        batch = synth.make_batch(conc, B, NPPF0, ncmp=NCMP, vocab_size=VOCAB, prop_dim=cfg.mdl.prop_feat_dim,
                                 seg_dim=cfg.mdl.seg_feat_dim, seed=3, ragged=True)
        eng = engine_mod.VogEngine(cfg, comm_for(c))
        eng.load_state_dict(sd)
        o = oracle_run(cfg, sd, batch, c)
        keys = ("mdl_outs", "mdl_outs_eval", "scores", "boxes", "indexs", "vidf_outs", "fin_scores", "fin_scores_loss")
        _BUILT[key] = (eng, cfg, sd, batch, c, _OracleGolden({k: o[k].numpy() for k in keys if k in o}))
    _BUILT[key][0].set_option("fused_tail", 1)
    return _BUILT[key]


def to_dev(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}


# ---- 1: the operator ---------------------------------------------------------------------------------------------------------
OP_CASES = [(77, 256, 384, "plain"), (200, 384, 384, "plain"),
            (77, 256, 320, "plain"), (200, 256, 256, "plain"), (200, 384, 640, "plain"), (77, 384, 512, "plain"),
            (200, 384, 384, "vislang"), (200, 256, 384, "vislang"), (200, 384, 384, "score"), (200, 256, 384, "score")]


# 65 row blocks: every k-step rotation. f16 only: the rotation is index arithmetic that both operand types share, and what the
# bound measures here is rounding flips - a flipped x1 / hidden element moves its whole row by (one 16-bit ulp) x (a W1 / W2
# column), which GROWS as the width shrinks (W2 entries ~ 1 / sqrt(dh)) and is 8 x larger in bf16 than in f16. Measured at these
# two shapes: f16 252 / 389 of 4112 rows above 1e-4, maxima 7.2e-4 / 5.8e-4; bf16 35 / 59 rows, maxima 4.4e-3 / 3.8e-3 with the
# median row at 1e-6 - at this many rows bf16's flip tail crosses 4e-3 and says nothing about the rotation.
ROT_CASES = [(4112, 256, 384, "plain", "f16"), (4112, 384, 384, "plain", "f16")]


@pytest.mark.parametrize("M,d,kwo,mode,dtype", [c + (t,) for c in OP_CASES for t in ("bf16", "f16")] + ROT_CASES)
def test_tail_operator_matches_torch_chain(M, d, kwo, mode, dtype):
    """Inputs, rounding points, seed rule and bounds of tests/test_gpu_ops.py::test_tx_tail_matches_torch_chain."""
    torch.manual_seed(M + d)
    lib, T = L.load(), t16(dtype)
    dh = d // 2
    assert lib.vog_tx_tail_supported(d, dh, kwo) == 1
    attn = (torch.randn(M, kwo, device="cuda") * 0.5).to(T)
    wo = torch.randn(d, kwo) / math.sqrt(kwo)
    w1 = torch.randn(dh, d) / math.sqrt(d)
    w2 = torch.randn(d, dh) / math.sqrt(dh)
    b1, b2 = torch.randn(dh, device="cuda") * 0.1, torch.randn(d, device="cuda") * 0.1
    g1, be1 = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    g2, be2 = 1 + 0.1 * torch.randn(d, device="cuda"), 0.1 * torch.randn(d, device="cuda")
    a = L.TxTailArgs()
    a.attn16, a.kwo = L.ptr(attn), kwo
    wo_p, w1_p, w2_p = _pack32(wo, dtype), _pack32(w1, dtype), _pack32(w2, dtype)
    a.wo_p, a.w1_p, a.w2_p = L.ptr(wo_p), L.ptr(w1_p), L.ptr(w2_p)
    a.ln1g, a.ln1b, a.b1, a.b2, a.ln2g, a.ln2b = L.ptr(g1), L.ptr(be1), L.ptr(b1), L.ptr(b2), L.ptr(g2), L.ptr(be2)
    n_vid, nfrm, nsrl, nppf = 1, 2, 5, 20
    if mode == "plain":
        res = torch.randn(M, d, device="cuda")
        a.residual, a.ldr = L.ptr(res), d
    else:
        assert n_vid * nfrm * nsrl * nppf == M
        dv, dl = (256, 128) if d == 384 else (192, 64)
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
    scr = torch.empty(max(int(lib.vog_tx_tail_scratch_bytes(M, d)), 16), dtype=torch.uint8, device="cuda")
    a.x1_scratch = L.ptr(scr)
    a.M, a.d, a.dh, a.dtype = M, d, dh, DT[dtype]
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
        cmp_msk = torch.tensor([[1, 0, 1, 1]], device="cuda", dtype=torch.int64)
        outs = torch.full((n_vid, 1, nsrl, nfrm * nppf), float("nan"), device="cuda")
        outs_eval = torch.full_like(outs, float("nan"))
        sa = L.ScoreArgs()
        sa.w2, sa.b2, sa.arg_msk, sa.cmp_msk = L.ptr(wl2), L.ptr(bl2), L.ptr(arg_msk), L.ptr(cmp_msk)
        sa.outs, sa.outs_eval = L.ptr(outs), L.ptr(outs_eval)
        sa.n_vid, sa.nfrm, sa.nppf, sa.nsrl, sa.dh = n_vid, nfrm, nppf, nsrl, 256
        sa.conc_type, sa.ncmp, sa.nc_v, sa.nvl, sa.nfrm0, sa.nppf0 = L.CONC_TYPE["spat"], 4, 1, 1, nfrm, 5
        a.wl_p, a.bl, a.score, a.head_dtype = L.ptr(wl_p), L.ptr(bl), C.addressof(sa), L.VOG_F16
    else:
        a.y32, a.y16 = L.ptr(y32), L.ptr(y16)
    L.check(lib.vog_tx_tail_fwd(C.byref(a), L.stream_ptr()), "tx_tail")
    torch.cuda.synchronize()
    if mode != "score":
        e32, e16 = (y32 - y).abs().max().item(), (y16.float() - y).abs().max().item()
        # (a 16-bit rounding flip of one x1 / hidden element moves ONE row: rows above 1e-4 and the median row say which it is)
        rows = (y32 - y).abs().amax(1)
        print(f"tail d={d} kwo={kwo} M={M} {mode} {dtype}: y32 max abs err {e32:.3e}, y16 {e16:.3e}; rows above 1e-4: "
              f"{int((rows > 1e-4).sum())} of {M}, median row {rows.median().item():.2e}")
        assert e32 <= 4e-3, e32
        assert e16 <= 3e-2, e16
        return
    h1 = torch.relu(y.half().float() @ wl.cuda().half().float().t() + bl)
    logit = (h1 @ wl2 + bl2).view(n_vid, nfrm, nsrl, nppf).permute(0, 2, 1, 3).reshape(n_vid, 1, nsrl, nfrm * nppf)
    cmp = (torch.arange(nfrm * nppf, device="cuda") // 5) % 4
    ref_eval = torch.sigmoid(logit) * arg_msk.view(n_vid, 1, nsrl, 1).float() * cmp_msk[:, cmp].view(n_vid, 1, 1, -1).float()
    el, ee = (outs - logit).abs().max().item(), (outs_eval - ref_eval).abs().max().item()
    print(f"tail d={d} kwo={kwo} M={M} score {dtype}: logit max abs err {el:.3e}, outs_eval {ee:.3e}")
    assert el <= 4e-3, el
    assert ee <= 1.5e-3, ee
    assert torch.all(outs_eval[ref_eval == 0] == 0)


# ---- 2: probe and entry ------------------------------------------------------------------------------------------------------
def _bare_args(M, d, dh, kwo, bufs):
    a = L.TxTailArgs()
    a.attn16, a.kwo = L.ptr(bufs["h"]), kwo
    a.wo_p, a.w1_p, a.w2_p = L.ptr(bufs["h"]), L.ptr(bufs["h"]), L.ptr(bufs["h"])
    a.ln1g, a.ln1b, a.b1, a.b2, a.ln2g, a.ln2b = (L.ptr(bufs["f"]),) * 6
    a.residual, a.ldr = L.ptr(bufs["f"]), d
    a.y32 = L.ptr(bufs["y"])
    a.x1_scratch = L.ptr(bufs["f"])
    a.M, a.d, a.dh, a.dtype = M, d, dh, L.VOG_BF16
    return a


def test_probe_and_entry_agree():
    lib, M = L.load(), 64
    bufs = {"h": torch.zeros(1024 * 1024, dtype=torch.bfloat16, device="cuda"), "f": torch.zeros(M * 1024, device="cuda"),
            "y": torch.empty(M * 1024, device="cuda")}
    for d in (256, 320, 384, 512):
        for dh in (d // 2, d // 2 - 32):
            for kwo in (256, 320, 384, 448, 512, 640):
                bufs["y"].fill_(float("nan"))
                rc = lib.vog_tx_tail_fwd(C.byref(_bare_args(M, d, dh, kwo, bufs)), L.stream_ptr())
                torch.cuda.synchronize()
                want = lib.vog_tx_tail_supported(d, dh, kwo)
                assert (rc == 0) == (want == 1), (d, dh, kwo, rc, want)
                assert bool(torch.isnan(bufs["y"][:M * d]).any()) == (want == 0), (d, dh, kwo)     # launched exactly where it is taken
    # hi + lo operands: no body at the narrow widths - an error, and nothing runs
    for d, kwo in ((256, 384), (384, 384)):
        a = _bare_args(M, d, d // 2, kwo, bufs)
        a.attn16_lo = a.wo_p_lo = a.w1_p_lo = a.w2_p_lo = L.ptr(bufs["h"])
        bufs["y"].fill_(float("nan"))
        assert lib.vog_tx_tail_fwd(C.byref(a), L.stream_ptr()) != 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(bufs["y"]).all())


# ---- 3: launch trace (nothing runs) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdl,conc", [("vog", "spat"), ("vog", "sep"), ("vgrnd", "spat")])
def test_launch_trace(mdl, conc):
    eng, cfg, sd, batch, c, _ = w128(mdl, conc)
    dev = to_dev(batch)
    tr = flat(trace(eng, dev, None))
    gone = [f"obj_{s}" for s in UNFUSED]
    if mdl == "vog":
        assert "obj_tail" in tr and "mul_tail" in tr, tr
        gone += [f"mul_{s}" for s in UNFUSED] + ["lin2", "score"]
    else:
        assert "obj_tail" in tr and "lin2" in tr and "score" in tr and "mul_tail" not in tr, tr
    assert not [s for s in gone if s in tr], tr
    eng.set_option("fused_tail", 0)
    off = flat(trace(eng, dev, None))
    eng.set_option("fused_tail", 1)
    assert "obj_tail" not in off and "mul_tail" not in off and all(f"obj_{s}" in off for s in UNFUSED), off


# ---- 4: the whole forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdl,conc", MODELS)
def test_forward_vs_oracle_with_the_unfused_control(mdl, conc):
    eng, cfg, sd, batch, c, g = w128(mdl, conc)
    name = f"w128/{mdl}_{conc}"
    dev = to_dev(batch)
    before = {k: v.clone() for k, v in dev.items()}
    ncmp = batch["new_srl_idxs"].shape[1]
    eng.set_option("fused_tail", 0)
    ctl = eng.forward(dev)
    torch.cuda.synchronize()
    ctl = {k: v.clone() for k, v in ctl.items() if isinstance(v, torch.Tensor)}
    eng.set_option("fused_tail", 1)
    assert "obj_tail" in flat(trace(eng, dev, None))
    out = eng.forward(dev)
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}
    for k in before:
        assert torch.equal(before[k], dev[k]), k
    assert bool(torch.isfinite(out["mdl_outs"]).all()) and bool(torch.isfinite(ctl["mdl_outs"]).all())
    # the control first: if IT misses the bound, the figures of both are in the output
    _check_against(name + " fused_tail=0 (control)", ctl, eng.unpack_pred(ctl["pred_rec"], ncmp), g, None, tol_rel=1e-3, tol_logit=6e-3)
    _check_against(name + " fused_tail=1", out, eng.unpack_pred(out["pred_rec"], ncmp), g, None, tol_rel=1e-3, tol_logit=6e-3)
    dl = (out["mdl_outs"] - ctl["mdl_outs"]).abs().max().item()
    print(f"{name}: fused vs unfused mdl_outs max abs {dl:.3e}")
    assert dl <= 1.5e-3, dl
    # a captured slot's second replay equals the eager forward bit for bit
    slot = eng.make_slot(dev, graph=True)
    slot.launch()
    torch.cuda.synchronize()
    rep = slot.launch()
    torch.cuda.synchronize()
    slot.check()
    for k in OUT_KEYS:
        assert torch.equal(rep[k], out[k]), (name, k)


@pytest.mark.parametrize("mdl,conc", [("vog", "spat"), ("vgrnd", "spat")])
def test_paired_obj_tail_equals_separate_launches(mdl, conc):
    """lstm_layer#1 || obj_tail in one grid (csrc/pair.hip: the 256-wide body is registered) runs the stand-alone bodies:
    bit-identical outputs with the pair formed (pair_mask 15), left as two launches (13) and with pairing off"""
    eng, cfg, sd, batch, c, _ = w128(mdl, conc)
    dev = to_dev(batch)
    eng.set_option("enc_lean", 1)            # (the encoder form otherwise follows the pairing decision)
    print("steps:", " ".join(trace(eng, dev, None)))
    ref = {k: v.clone() for k, v in eng.forward(dev).items() if k in OUT_KEYS}
    try:
        for opt, v in (("pair_mask", 13), ("pair_launches", 0)):
            eng.set_option(opt, v)
            out = eng.forward(dev)
            torch.cuda.synchronize()
            for k in OUT_KEYS:
                assert torch.equal(out[k], ref[k]), (opt, k)
    finally:
        eng.set_option("pair_mask", 15)
        eng.set_option("pair_launches", 1)
        eng.set_option("enc_lean", -1)


# ---- 5: plan gate------------------------------------------------------------------------------------------------------------
def test_hi_lo_plan_stays_off():
    eng = w128("vog", "spat")[0]
    assert eng.lib.vog_ctx_split_supported(eng.ctx, 4) == 0
    assert eng.plan == "f16"


# ---- 6: weight images and refresh ----------------------------------------------------------------------------------------------
def test_images_exist_and_refresh_from_device_equals_load_state_dict():
    A, cfg, sd, batch, c, _ = w128("vog", "spat")
    rows = {r["name"]: r for r in A.weight_images()}
    assert int(A.desc.obj_heads) == int(A.desc.mul_heads) == 3          # 86 / 128 columns per head, padded to 128: kwo = 384
    for pre, d in (("obj_txf", 256), ("mult_txf", 384)):
        assert rows[f"{pre}.0.wo_p"]["bytes"] == d * 384 * 2 and rows[f"{pre}.0.wo_p"]["kind"] == "frag32"
        assert rows[f"{pre}.0.w1_p"]["bytes"] == rows[f"{pre}.0.w2_p"]["bytes"] == d * (d // 2) * 2
    assert rows["w_lin2_p"]["bytes"] == 256 * 384 * 2 and rows["w_lin2_p"]["kind"] == "frag32"
    assert not [n for n in rows if n.endswith("_lo")]
    other = synth.init_state_dict(cfg, VOCAB, seed=2, perturb_ln=True)
    Bn = engine_mod.VogEngine(cfg, comm_for(c))
    Bn.load_state_dict(other)
    dev = to_dev(batch)
    ob0 = Bn.forward(dev)["mdl_outs"].clone()
    how = Bn.refresh_from_device({k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sd.items()})
    assert how == "in_place"
    oa, ob = A.forward(dev), Bn.forward(dev)
    torch.cuda.synchronize()
    assert not torch.equal(ob0, oa["mdl_outs"])
    for k in OUT_KEYS:
        assert torch.equal(oa[k], ob[k]), k


# ---- 7: ObjBank rows -----------------------------------------------------------------------------------------------------------
def test_obj_rows_forward_equals_the_raw_forward():
    eng, cfg, sd, batch, c, _ = w128("vog", "sep")
    assert eng.obj_band_rows() == 512
    dev = to_dev(batch)
    assert B * NCMP * int(eng.desc.nfrm0) * NPPF0 == 400          # the batch's obj_tx rows: one rotation band
    T = int(batch["srl_arg_word_mask_len"].max())
    obj = objed(eng, dev)
    raw = {k: v.clone() for k, v in eng.forward(dev, T=T).items() if isinstance(v, torch.Tensor)}
    out = eng.forward(obj, T=T)
    torch.cuda.synchronize()
    for k in OUT_KEYS + ("vidf_outs",):
        assert torch.equal(out[k], raw[k]), k
    tr = flat(trace(eng, obj, T))
    assert "obj_tail" not in tr and "mul_tail" in tr, tr
