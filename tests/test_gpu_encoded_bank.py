"""-m gpu: forwards from encoder outputs (vog_batch.enc_prop / enc_seg -> the `vis_concat` step) and the encoded feature bank
(dat_loader_simple.EncodedBank, filled through vog_ctx_encode_videos): everything the raw path computes from
pad_region_feature / seg_feature_for_frms, the encoded path computes bit for bit - the three forms of prop_seg, the model
outputs, the prediction records, the loss and the pickle - and the encoded runs hold the bounds of tests/test_gpu_forward.py
against the reference goldens."""
import ctypes as C
import importlib
import pickle

import numpy as np
import pytest
import torch

from oracle import cases
from oracle import vog_oracle as vo
from tests.gpu_util import L, build_engine, comm_for, engine_mod, t16
from tests.gpu_util import encoded as _encoded, flat as _flat, index_batches as _index_batches, trace as _trace, video_pool as _pool
from tests.test_gpu_forward import _check_against

pytestmark = pytest.mark.gpu

dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
synth = importlib.import_module("vognet-pytorch_amd.synth")

FEATS = ("pad_region_feature", "seg_feature_for_frms")
ENC = engine_mod.ENC_KEYS
OUT_KEYS = ("mdl_outs", "mdl_outs_eval", "pred_rec")
SEP_KEYS = ("vidf_outs", "fin_scores_loss", "fin_scores")
LANG_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
             "srl_arg_inds_msk", "num_cmp_msk")
ENCODER_STEPS = ("vis_enc", "seg_rep", "prop_enc", "seg_enc", "enc_finish")
CFG2 = "full/cfg2_vog_spat_gt5_bs4"
FUSED_SMALL = "fused_small"               # the smallest shape the fused encoder kernel takes; no golden (built here)


def _engine(name, tx_dtype=None):
    if name != FUSED_SMALL:
        return build_engine(name, tx_dtype=tx_dtype, cached=True)
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"mdl.name": "vog", "ds.conc_type": "spat", **cases.REL, **cases.SMALL_DIMS,
                              "mdl.prop_feat_dim": 256, "mdl.seg_feat_dim": 256, "mdl.vsrl.prop_encode_size": 32,
                              "mdl.vsrl.seg_encode_size": 32})
    c = {"vocab": 50, "nppf0": 5}
    sd = synth.init_state_dict(cfg, 50, seed=1, perturb_ln=True)
    batch = synth.make_batch("spat", 1, 5, ncmp=2, vocab_size=50, prop_dim=256, seg_dim=256, seed=3, ragged=True)
    eng = engine_mod.VogEngine(cfg, comm_for(c))
    eng.load_state_dict(sd)
    return eng, cfg, sd, batch, c, {k: torch.from_numpy(v).cuda() for k, v in batch.items()}


def _stages(eng, dev, T):
    B, ncmp, _, NP = eng._geometry(dev)
    d = eng.desc
    rows, dobj = B * (ncmp if eng.sep else 1) * NP, d.prop_enc + d.seg_enc
    names = ["prop_seg", "prop_seg16"] + (["prop_seg16_lo"] if eng.plan == "split" else [])
    return {n: eng.stage(B, ncmp, T, n, torch.float32 if n == "prop_seg" else torch.int16, (rows, dobj)).clone() for n in names}


# ---- 1: the three forms of prop_seg ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tx", [("small/vog_spat", None), (FUSED_SMALL, None), ("small/vog_spat_p7", None),
                                     ("full/cfg2_sharp16", None), (CFG2, "bf16")])
def test_prop_seg_stages_equal_the_encoders(name, tx):
    """Raw forward, then the encoded forward of the same batch in the same workspace: prop_seg, prop_seg16 and, on the hi + lo
    plan, prop_seg16_lo hold the same bits. small/vog_spat: cast + GEMM encoders; fused_small: the fused kernel at its smallest
    shape (feature dims 256, encode sizes 32, B = 1, ncmp = 2); small/vog_spat_p7: nppf0 = 7, 560 rows = 8.75 row blocks of
    the concat kernel (4 threads per row, 64 rows per block); full/cfg2_sharp16 plans `split`."""
    eng, cfg, sd, batch, c, dev = _engine(name, tx)
    T = int(batch["srl_arg_word_mask_len"].max())
    raw_trace = _flat(_trace(eng, dev, T))
    assert ("vis_enc" in raw_trace) == (name in (FUSED_SMALL, "full/cfg2_sharp16", CFG2)) and ("prop_enc" in raw_trace) == (name.startswith("small/"))
    if name == "full/cfg2_sharp16":
        assert eng.plan == "split"
    enc = _encoded(eng, dev)
    eng.forward(dev, T=T)
    torch.cuda.synchronize()
    want = _stages(eng, dev, T)
    for n in want:                                           # (the encoded run has to write them, not inherit them)
        eng.stage(*eng._geometry(dev)[:2], T, n, torch.uint8, (want[n].numel() * want[n].element_size(),)).fill_(0xA5)
    eng.forward(enc, T=T)
    torch.cuda.synchronize()
    got = _stages(eng, dev, T)
    assert set(got) == set(want) and len(want) == (3 if eng.plan == "split" else 2)
    for n in want:
        assert torch.equal(got[n], want[n]), (name, n)
    assert want["prop_seg"].abs().sum() > 0
    # and the table is what the oracle's encoders give, to the operand precision (fp32 reference on 16-bit operands)
    d = eng.desc
    ref = torch.relu(dev["pad_region_feature"].reshape(-1, d.prop_dim).half().float() @ torch.from_numpy(sd["prop_encoder.0.weight"]).cuda().half().float().T
                     + torch.from_numpy(sd["prop_encoder.0.bias"]).cuda())
    assert torch.allclose(enc[ENC[0]].reshape(-1, d.prop_enc), ref, rtol=2e-3, atol=2e-3)


def _expected_concat(ep, es, nppf0, dt):
    o = torch.cat([ep, es.repeat_interleave(nppf0, dim=0)], dim=1)
    hi = o.to(dt)
    lo = (o - hi.float()).to(dt)
    return o, hi.view(torch.int16), lo.view(torch.int16)


@pytest.mark.parametrize("prop_enc,seg_enc,ldc,nppf0,rows,dt", [
    (6, 9, 15, 7, 259, "f16"),            # odd sizes, odd pitch: one element per thread; 259 rows = 15.2 blocks
    (6, 10, 19, 5, 35, "bf16"),           # the same with a pitch wider than the row
    (12, 20, 32, 7, 63, "f16"),           # multiples of 4, not of 8: 16-byte loads, 8-byte 16-bit stores
    (16, 8, 24, 100, 300, "bf16"),        # multiples of 8: 16-byte stores of the 16-bit rows; nppf0 = 100
    (16, 16, 32, 5, 10, "f16")])          # fewer elements than one block
def test_vis_concat_operator_sizes_outside_the_models(prop_enc, seg_enc, ldc, nppf0, rows, dt):
    """vog_vis_concat on its own at the sizes no context can have (vog_ctx_create asks for encode sizes % 8 == 0): the scalar
    path, the 4- and the 8-column paths, row pitch > row width (the gap is not written), a last partial block. Expected values
    from torch: RNE casts, the remainder from the exact fp32 difference."""
    g = torch.Generator().manual_seed(prop_enc * 100 + seg_enc)
    ep = (torch.randn(rows, prop_enc, generator=g) * 3).cuda()
    es = (torch.randn(rows // nppf0, seg_enc, generator=g) * 3).cuda()
    ep[0, 0], ep[1, 1], es[0, 0] = 0.0, 65504.0 if dt == "f16" else 3e38, 1e-7       # zero, the largest finite, a subnormal result
    o, hi, lo = _expected_concat(ep, es, nppf0, t16(dt))
    c32 = torch.full((rows, ldc), -7.0, device="cuda")
    c16 = torch.full((rows, ldc), 0x1234, dtype=torch.int16, device="cuda")
    clo = torch.full((rows, ldc), 0x1234, dtype=torch.int16, device="cuda")
    a = L.VisconcatArgs()
    a.enc_prop, a.enc_seg, a.c32, a.c16, a.c16_lo = (t.data_ptr() for t in (ep, es, c32, c16, clo))
    a.ldc, a.c16_dtype, a.n_rows, a.nppf0, a.prop_enc, a.seg_enc = ldc, L.DTYPE[dt], rows, nppf0, prop_enc, seg_enc
    L.check(L.load().vog_vis_concat(C.byref(a), L.stream_ptr()), "vog_vis_concat")
    torch.cuda.synchronize()
    w = prop_enc + seg_enc
    assert torch.equal(c32[:, :w], o) and torch.equal(c16[:, :w], hi) and torch.equal(clo[:, :w], lo)
    assert bool((c32[:, w:] == -7.0).all()) and bool((c16[:, w:] == 0x1234).all()) and bool((clo[:, w:] == 0x1234).all())
    assert bool((lo != 0).any())
    # optional outputs: the 16-bit rows alone
    c16.fill_(0)
    a.c32, a.c16_lo = None, None
    L.check(L.load().vog_vis_concat(C.byref(a), L.stream_ptr()), "vog_vis_concat")
    torch.cuda.synchronize()
    assert torch.equal(c16[:, :w], hi) and bool((c32[:, :w] == o).all())


# ---- 2: the whole forward --------------------------------------------------------------------------------------------------
WHOLE = [("small/vog_spat", None), ("small/vog_temp", None), ("small/vog_sep", None), ("small/igrnd_spat", None),
         ("small/vog_spat_3layers", None), ("full/cfg2_sharp16", None), (CFG2, "f16"), (CFG2, "bf16")]


@pytest.mark.parametrize("name,tx", WHOLE)
def test_whole_forward_equals_the_raw_path(name, tx):
    """mdl_outs, mdl_outs_eval, the prediction records and the sep outputs (the verb head reads the segment mean out of
    prop_seg) from encoded inputs == from raw inputs, eager and from a graph slot; the encoded outputs hold the bounds of
    tests/test_gpu_forward.py against the reference golden."""
    eng, cfg, sd, batch, c, dev = _engine(name, tx)
    if name == "full/cfg2_sharp16":
        assert eng.plan == "split"
    T = int(batch["srl_arg_word_mask_len"].max())
    enc = _encoded(eng, dev)
    keys = OUT_KEYS + (SEP_KEYS if eng.sep else ())
    raw_out = eng.forward(dev, T=T)
    torch.cuda.synchronize()
    raw_out = {k: raw_out[k].clone() for k in keys}
    before = {k: v.clone() for k, v in enc.items()}
    out = eng.forward(enc, T=T)
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(out[k], raw_out[k]), (name, k)
    slot = eng.make_slot(enc, T=T, graph=True)
    sout = slot.launch()
    torch.cuda.synchronize()
    slot.check()
    for k in keys:
        assert torch.equal(sout[k], raw_out[k]), (name, "slot", k)
    for k in before:
        assert torch.equal(before[k], enc[k]), k
    assert torch.isfinite(out["mdl_outs"]).all()
    ncmp = batch["new_srl_idxs"].shape[1]
    _check_against(name, out, eng.unpack_pred(out["pred_rec"], ncmp), np.load(cases.golden_path(name)), None, tol_rel=1e-3, tol_logit=6e-3)


# ---- 3: the launch trace ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small/vog_spat", CFG2, "full/cfg3_vog_temp_gt5_bs8", "small/igrnd_spat"])
def test_launch_trace_of_an_encoded_batch(name):
    """`vis_concat` in place of every encoder step; the feature cast is gone with them (small: the GEMM form's operands); the
    BiLSTM layer that shared its launch with the encoders launches alone, the visual steps that followed the pair still follow
    it, and every later pair keeps its partner. The default trace of the same batch is what it was."""
    eng, cfg, sd, batch, c, dev = _engine(name)
    T = int(batch["srl_arg_word_mask_len"].max())
    raw = _trace(eng, dev, T)
    enc = _trace(eng, _encoded(eng, dev), T)
    assert _trace(eng, dev, T) == raw
    fe = _flat(enc)
    assert fe.count("vis_concat") == 1 and not set(fe) & set(ENCODER_STEPS) and "vis_prep" not in fe
    assert set(_flat(raw)) & set(ENCODER_STEPS) and "vis_concat" not in _flat(raw)
    # everything else is the same launches in the same order
    strip = lambda t: [p for p in _flat(t) if p not in ENCODER_STEPS + ("vis_concat",)]
    assert strip(enc) == strip(raw)
    if name == CFG2:
        assert raw[:2] == ["prep", "lstm_layer+vis_enc"] and enc[:3] == ["prep", "lstm_layer", "vis_concat"]
        assert [n for n in enc if "+" in n] == [n for n in raw if "+" in n and "vis_enc" not in n] and len(enc) == len(raw) + 1
    i = fe.index("vis_concat")
    consumers = [p for p in fe if p in ("obj_qkv", "mul_pv", "vislang", "pred_cmp")]
    assert consumers and all(fe.index(p) > i for p in consumers)


# ---- 4: EncodedBank ----------------------------------------------------------------------------------------------------------
def _banks(eng, cfg, c, batch, nv=13, seed=17):
    """13 videos: three full chunks of B * ncmp = 8 / 4 ... and a short last one for every case below."""
    raw = dls.FeatureBank(cfg, comm_for(c), nv, dtype="f32", n_gt=8)
    raw.put(0, _pool(nv, cfg, c, seed))
    Bq, ncmp = batch["num_cmp_msk"].shape
    enc = dls.EncodedBank.encode(raw, eng, Bq, ncmp)
    return raw, enc


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep"])
def test_encoded_bank_loader_equals_the_raw_bank_loader(name):
    eng, cfg, sd, batch, c, dev = build_engine(name)
    T = int(batch["srl_arg_word_mask_len"].max())
    raw, enc = _banks(eng, cfg, c, batch)
    d = eng.desc
    assert isinstance(enc, dls.FeatureBank) and (enc.prop_dim, enc.seg_dim, enc.dtype) == (d.prop_enc, d.seg_enc, "f32")
    assert enc.nbytes == enc.V * dls.EncodedBank.bytes_per_video(c["nppf0"], d.prop_enc, d.seg_enc, 8) < raw.nbytes
    assert (enc.epoch, enc.plan, enc.geometry) == (eng.weights_epoch, eng.plan, tuple(batch["num_cmp_msk"].shape))
    assert enc.lossless_for(eng) and enc.fwd_keys == ("pad_proposals",) + ENC and enc.encode_seconds > 0
    with pytest.raises(TypeError):
        enc.put(0, {})
    ibs = _index_batches(batch, cfg, c, raw.V, 3)
    keys = OUT_KEYS + (SEP_KEYS if eng.sep else ())
    n = 0
    for rb, eb in zip(raw.loader(ibs), enc.loader(ibs)):
        assert set(rb) - set(FEATS) == set(eb) - set(ENC) and set(FEATS) <= set(rb) and set(ENC) <= set(eb) and not set(FEATS) & set(eb)
        for k in set(rb) - set(FEATS):                                  # loss keys, proposals, language: identical
            assert torch.equal(rb[k], eb[k]), k
        o_raw, o_enc = eng.forward(rb, T=T), eng.forward(eb, T=T)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(o_raw[k], o_enc[k]), (n, k)
        n += 1
    assert n == 3
    enc.check()
    # the same rows from host items, the raw features never a bank on the device
    pool = _pool(raw.V, cfg, c, 17)
    Bq, ncmp = batch["num_cmp_msk"].shape
    chunks = [(s0, {k: v[s0:s0 + 5] for k, v in pool.items()}) for s0 in range(0, raw.V, 5)]
    enc2 = dls.EncodedBank.from_items(cfg, comm_for(c), raw.V, chunks, eng, Bq, ncmp, n_gt=8)
    for k in enc.tab:
        assert torch.equal(enc.tab[k], enc2.tab[k]), k
    with pytest.raises(L.VogError, match="raw bank"):
        enc2.refresh()


def test_encoded_bank_guards_a_bad_index():
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_spat", cached=True)
    raw, enc = _banks(eng, cfg, c, batch)
    Bq, ncmp = batch["num_cmp_msk"].shape
    idx = np.random.default_rng(5).integers(0, raw.V, size=(Bq, ncmp)).astype(np.int32)
    good = enc(torch.from_numpy(idx).cuda(), with_loss_keys=False)
    idx[1, 2] = raw.V
    with pytest.raises(ValueError, match="outside"):
        enc(torch.from_numpy(idx), with_loss_keys=False)
    got = enc(torch.from_numpy(idx).cuda(), with_loss_keys=False)
    torch.cuda.synchronize()
    d = eng.desc
    # spat: video 2 of query 1 owns proposals [2 * nppf0, 3 * nppf0) of every frame
    r = got[ENC[0]][1].reshape(d.nfrm0, ncmp, d.nppf0, d.prop_enc)
    assert not r[:, 2].any() and torch.equal(r[:, :2], good[ENC[0]][1].reshape(d.nfrm0, ncmp, d.nppf0, d.prop_enc)[:, :2])
    assert torch.equal(got[ENC[0]][0], good[ENC[0]][0]) and bool(good[ENC[0]][1].reshape(d.nfrm0, ncmp, d.nppf0, d.prop_enc)[:, 2].any())
    with pytest.raises(L.VogError, match="outside"):
        enc.check()
    enc.check()                                                        # reported once


def test_encoded_bank_goes_stale_with_the_weights_and_refreshes():
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_spat")
    T = int(batch["srl_arg_word_mask_len"].max())
    raw, enc = _banks(eng, cfg, c, batch)
    ibs = _index_batches(batch, cfg, c, raw.V, 1)
    old = enc.tab["pad_region_feature"].clone()
    sd2 = dict(sd)
    rng = np.random.default_rng(9)
    for k in ("prop_encoder.0.weight", "seg_encoder.0.weight", "prop_encoder.0.bias"):
        sd2[k] = (sd[k] + 0.05 * rng.standard_normal(sd[k].shape)).astype(np.float32)
    eng.load_state_dict(sd2)
    assert enc.stale() and not enc.lossless_for(eng)
    with pytest.raises(L.VogError, match="refresh"):
        enc.check()
    with pytest.raises(L.VogError, match="refresh"):                   # (stale until refreshed: not a once-only report)
        next(iter(enc.loader(ibs))), enc.check()
    assert enc.refresh() is enc and not enc.stale() and enc.epoch == eng.weights_epoch
    assert not torch.equal(old, enc.tab["pad_region_feature"])
    enc.check()
    rb, eb = next(iter(raw.loader(ibs))), next(iter(enc.loader(ibs)))
    o_raw, o_enc = eng.forward(rb, T=T), eng.forward(eb, T=T)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert torch.equal(o_raw[k], o_enc[k]), k
    # the reference for the new weights: the oracle's forward on the raw batch
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    host = {k: rb[k].cpu().numpy() for k in batch}
    with torch.no_grad():
        ref = vo.forward(oc, vo.to_torch(sd2), vo.to_torch(host))
    assert float((o_enc["mdl_outs"].cpu() - torch.as_tensor(np.asarray(ref["mdl_outs"]))).abs().max()) <= 6e-3


# ---- 5: fed slots and the validation graph -----------------------------------------------------------------------------------
def test_fed_pipeline_from_an_encoded_bank():
    """8 steps with changing indices through FedPipeline(..., assembler=encoded): every launch equals the eager forward on the
    encoded batch of the same videos, which equals the eager forward on the raw batch."""
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_spat", cached=True)
    T = int(batch["srl_arg_word_mask_len"].max())
    raw, enc = _banks(eng, cfg, c, batch)
    Bq, ncmp = batch["num_cmp_msk"].shape
    lang = {k: dev[k] for k in LANG_KEYS}
    ex = enc(torch.zeros(Bq, ncmp, dtype=torch.int32).cuda(), with_loss_keys=False)
    ex.pop("_keepalive")
    assert set(ex) == set(enc.fwd_keys)
    ex.update(lang)
    spec = {"vid_index": np.zeros((Bq, ncmp), np.int32), **{k: np.zeros_like(batch[k]) for k in LANG_KEYS}}
    pipe = engine_mod.FedPipeline(eng, ex, spec, assembler=enc, streams=2, slots_per_stream=2, T=T)
    assert set(pipe.slots[0].fed_keys) == set(enc.fwd_keys) | set(LANG_KEYS)
    with pytest.raises(ValueError, match="other feature keys"):        # a raw bank cannot feed a slot made from encodings
        eng.make_slot(ex, T=T, graph=True).feed_from(dls.PackedStaging(spec, n_dev=1), assembler=raw, via="device")
    rng = np.random.default_rng(21)
    first = None
    for i in range(8):
        idx = rng.integers(0, raw.V, size=(Bq, ncmp)).astype(np.int32)
        st = pipe.next_staging()
        st.fill({"vid_index": idx})
        st.fill({k: batch[k] for k in LANG_KEYS})
        sl = pipe.submit()
        pipe.done(sl).synchronize()
        got = {k: sl.out[k].clone() for k in OUT_KEYS}
        di = torch.from_numpy(idx).cuda()
        e_in, r_in = enc(di, with_loss_keys=False), raw(di, with_loss_keys=False)
        for k in enc.fwd_keys:
            assert torch.equal(sl.inp[k], e_in[k]), (i, k)
        o_enc = eng.forward({**lang, **{k: e_in[k] for k in enc.fwd_keys}}, T=T)
        o_raw = eng.forward({**lang, **{k: r_in[k] for k in raw.fwd_keys}}, T=T)
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.equal(got[k], o_enc[k]) and torch.equal(got[k], o_raw[k]), (i, k)
        first = first if first is not None else got
    assert not torch.equal(first["mdl_outs"], got["mdl_outs"])
    for sl in pipe.slots:
        sl.check()


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep"])
def test_evaluator_on_an_encoded_bank_equals_the_raw_bank(name, tmp_path, tmp_path_factory):
    """Evaluator.forward with val_graph, device metrics and the pickle on `encoded.loader(index_batches)`: the loss dict, the
    metric dict and the pickle bytes of the raw bank's run - through the fed slots' epilogue, with and without the query bank,
    and through the existing loop. Six batches of 4, the last a query short: the tail batch takes the eager calls at B = 3 with
    rows encoded for B = 4 (the GEMM encoders of these models tile 600 rows as they tile 800: the same bits)."""
    from tests import test_gpu_device_metrics as T
    from tests.test_gpu_val_graph import _run
    cfg, sd, comm, sel, dl = T.make_eval_set(name, tmp_path_factory.mktemp("ann_enc_" + name.replace("/", "_")), n_batches=6, B=4, distinct=5)
    assert len(dl) == 6 and int(dl[-1]["num_cmp_msk"].shape[0]) == 3
    nv, nppf0 = 24, comm["num_prop_per_frm"]
    it = synth.make_items(nv, 1, nppf0, prop_dim=int(cfg.mdl.prop_feat_dim), seg_dim=int(cfg.mdl.seg_feat_dim), seed=17)
    raw = dls.FeatureBank(cfg, comm, nv, dtype="f32")
    raw.put(0, {k: np.ascontiguousarray(it[k][:, 0]) for k in dls.BANK_KEYS})
    drop = set(dls.BANK_KEYS) | {"pad_frm_mask"}
    ibs = []
    for i, hb in enumerate(dl):
        b, ncmp = hb["num_cmp_msk"].shape
        idx = np.random.default_rng(300 + i).integers(0, nv, size=(b, ncmp)).astype(np.int32)
        ibs.append({**{k: v for k, v in hb.items() if k not in drop}, "vid_index": torch.from_numpy(idx)})
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    enc = dls.EncodedBank.encode(raw, mdl.engine(), *dl[0]["num_cmp_msk"].shape)
    ref = _run(cfg, mdl, evl, loss_fn, raw.loader(ibs), tmp_path / "raw", device_metrics=True, val_graph=True)
    assert ref[3] == "graph" and ref[0]["loss"] > 0 and ref[2] is not None and len(pickle.loads(ref[2])) == sum(len(b["sent_idx"]) for b in ibs)
    for tag, hip in (("graph", {"val_graph": True}), ("queries", {"val_graph": True, "query_bank": True}), ("eager", {})):
        got = _run(cfg, mdl, evl, loss_fn, enc.loader(ibs), tmp_path / tag, device_metrics=True, **hip)
        cfg.hip["query_bank"] = False
        assert got[3] == ("eager" if tag == "eager" else "graph"), tag
        assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2], (tag, got[0], ref[0], got[1], ref[1])
    enc.check()


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_restriction(tmp_path):
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_spat", cached=True)
    enc = _encoded(eng, dev)
    with pytest.raises(ValueError, match="make_batched takes raw features"):
        eng.make_batched([enc, enc])
    with pytest.raises(ValueError, match="make_group takes raw features"):
        eng.make_group([enc, enc])
    with pytest.raises(ValueError, match="pair"):
        eng.forward({k: v for k, v in enc.items() if k != ENC[1]})
    with pytest.raises(ValueError, match="not both"):
        eng.forward({**enc, FEATS[0]: dev[FEATS[0]]})
    with pytest.raises(ValueError, match="expected"):
        eng.forward({**enc, ENC[1]: enc[ENC[1]][:, :-1].contiguous()})
    with pytest.raises(ValueError, match="float32 tensor on the device"):
        eng.forward({**enc, ENC[0]: enc[ENC[0]].cpu()})
    # the fp32 plan reads raw features
    e32, *_ = build_engine("small/vog_spat", tx_dtype="f32", cached=True)
    assert e32.precise is not None and e32.plan == "f32"
    with pytest.raises(L.VogError, match="fp32 path reads raw features"):
        e32.forward(enc)
    with pytest.raises(L.VogError, match="fp32 path reads raw features"):
        e32.make_slot(enc)
    with pytest.raises(L.VogError, match="fp32 path reads raw features"):
        e32.encode_videos(dev[FEATS[0]].reshape(8, 50, -1), dev[FEATS[1]].reshape(8, 10, -1), 2, 4)
    # ... also when the plan is raised at run time: the observed logit scale escalates `auto` before the batch is read
    e2, *_ = build_engine("small/vog_spat")
    e2._stats[:2] = torch.tensor([1e9, 1e9]).view(torch.int32)
    with pytest.warns(UserWarning):
        with pytest.raises(L.VogError, match="fp32 path reads raw features"):
            e2.forward(enc)
    assert e2.plan == "f32"
    # training: the encoders are being trained
    tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
    sel = importlib.import_module("vognet-pytorch_amd.mdl_selector").get_mdl_loss_eval(cfg)
    comm = comm_for(c)
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    raw, ebank = _banks(eng, cfg, c, batch)
    ibs = _index_batches(batch, cfg, c, raw.V, 1)
    learn = tu.Learner(uid="enc", data=tu.DataWrap(path=tmp_path, train_dl=ebank.loader(ibs), valid_dl=ebank.loader(ibs)), mdl=mdl,
                       loss_fn=sel["loss"](cfg, comm), cfg=cfg, eval_fn=sel["eval"](cfg, comm, torch.device("cuda", 0)), comm=comm)
    eb = next(iter(ebank.loader(ibs)))
    with pytest.raises(L.VogError, match="trains prop_encoder"):
        learn.trainer.step(eb)
    with pytest.raises(L.VogError, match="trains prop_encoder"):
        learn.train_epoch()
    assert learn.trainer.num_it == 0


# ---- 7: the command line --------------------------------------------------------------------------------------------------------
def test_main_dist_feature_bank_enc(capsys, tmp_path):
    """`main_dist --only_val --feature_bank=enc` (full-size VOGNet, fused encoders, a short tail batch) prints the loss and the
    metrics of `--feature_bank=f16` and leaves the same pickle bytes; without `only_val` one epoch of `fit` trains from the raw
    bank and validates from the encoded one - whose loader ends in `check()`, so the run only passes if `Learner.validate`
    refreshed the rows after the epoch's weight sync."""
    import json
    main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
    over = {"mdl.name": "vog", "ds.conc_type": "spat", "mdl.obj_tx.use_rel": True, "mdl.mul_tx.use_rel": True, "train.bsv": 4}
    res = {}
    for kind in ("f16", "enc"):
        main_mod.main_dist("v_" + kind, only_val=True, synthetic_batches=3, feature_bank=kind, feature_bank_videos=32,
                           **over, **{"misc.tmp_path": str(tmp_path / kind)})
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{\"uid\"")][-1]
        res[kind] = (json.loads(line), open(tmp_path / kind / "predictions" / ("v_" + kind) / "valid_0.pkl", "rb").read())
    assert res["enc"][0]["feature_bank"] == "enc" and res["enc"][0]["queries"] == 11
    assert res["enc"][0]["val_loss"] == res["f16"][0]["val_loss"] and res["enc"][0]["val_acc"] == res["f16"][0]["val_acc"]
    assert res["enc"][1] == res["f16"][1] and len(pickle.loads(res["enc"][1])) == 11
    with pytest.raises(SystemExit):
        main_mod.main_dist("v_bad", only_val=True, feature_bank="bf16", **over, **{"misc.tmp_path": str(tmp_path / "bad")})
    hist = main_mod.main_dist("fit_enc", synthetic_batches=2, feature_bank="enc", feature_bank_videos=16, **over,
                              **{"misc.tmp_path": str(tmp_path / "fit"), "train.bs": 2, "train.epochs": 1})
    assert len(hist) == 1 and all(np.isfinite(v) for k, v in hist[0].items() if k.startswith(("trn_", "val_")))
