"""-m gpu: forwards from cached obj_tx rows (vog_batch.obj_out / enc_seg -> the `obj_restore` step) and the
object-transformer bank (dat_loader_simple.ObjBank, filled through vog_ctx_obj_videos), for sep / svsq models: everything the
raw path computes below mul_tx, the cached path holds bit for bit - the stack's fp32 rows, their 16-bit copies, the segment
columns of prop_seg, the model outputs, the prediction records, the loss and the pickle - and the cached runs hold the bounds
of tests/test_gpu_forward.py against the reference goldens."""
import ctypes as C
import importlib
import pickle

import numpy as np
import pytest
import torch

from oracle import cases
from tests.gpu_util import L, build_engine, comm_for, engine_mod, t16
from tests.gpu_util import flat as _flat, index_batches as _index_batches, objed as _objed, trace as _trace, video_pool as _pool
from tests.test_gpu_forward import _check_against

pytestmark = pytest.mark.gpu

dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
synth = importlib.import_module("vognet-pytorch_amd.synth")

FEATS = ("pad_region_feature", "seg_feature_for_frms")
OBJ = engine_mod.OBJ_KEYS
ENC = engine_mod.ENC_KEYS
OUT_KEYS = ("mdl_outs", "mdl_outs_eval", "pred_rec", "vidf_outs", "fin_scores_loss", "fin_scores")
LANG_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
             "srl_arg_inds_msk", "num_cmp_msk", "verb_ind_in_srl")
ENCODER_STEPS = ("vis_enc", "seg_rep", "prop_enc", "seg_enc", "enc_finish")
CFG5 = "full/cfg5_vog_svsq_gt5_bs16"
SHARP16 = "full/vog_sep_sharp16"
ROW_CASES = ["small/vog_sep", "small/vog_svsq", "small/vgrnd_sep", CFG5, SHARP16]


def _last(eng):
    return "obj_outA" if int(eng.desc.obj_layers) % 2 == 1 else "obj_outB"


def _stage(eng, dev, T, name, dtype):
    B, ncmp, _, NP = eng._geometry(dev)
    d = eng.desc
    return eng.stage(B, ncmp, T, name, dtype, (B * ncmp * NP, d.prop_enc + d.seg_enc))


# ---- 1: the operator ---------------------------------------------------------------------------------------------------------
def _expected_restore(x, es, nppf0, dt):
    hi = x.to(dt)
    lo = (x - hi.float()).to(dt)
    return hi.view(torch.int16), lo.view(torch.int16), es.repeat_interleave(nppf0, dim=0)


@pytest.mark.parametrize("d_obj,seg_enc,ldc,nppf0,rows,dt", [
    (15, 9, 15, 7, 259, "f16"),           # odd sizes, odd pitch: one element per thread; 259 rows = 15.2 blocks
    (16, 10, 19, 5, 35, "bf16"),          # the same with a pitch wider than the row
    (32, 20, 32, 7, 63, "f16"),           # multiples of 4, not of 8: 16-byte loads, 8-byte 16-bit stores
    (24, 8, 24, 100, 300, "bf16"),        # multiples of 8: 16-byte stores of the 16-bit rows; nppf0 = 100
    (32, 16, 32, 5, 10, "f16")])          # fewer elements than one block
def test_obj_restore_operator_sizes_outside_the_models(d_obj, seg_enc, ldc, nppf0, rows, dt):
    """vog_obj_restore on its own at sizes no context can have (vog_ctx_create asks for encode sizes % 8 == 0): the scalar path,
    the 4- and the 8-column paths, row pitch > row width (the gap is not written), a last partial block, each optional output
    left out in turn. Expected values from torch: RNE casts, the remainder from the exact fp32 difference. Planted: a zero, the
    largest finite value, and 1e-7 (a subnormal f16 result)."""
    g = torch.Generator().manual_seed(d_obj * 100 + seg_enc)
    x = (torch.randn(rows, d_obj, generator=g) * 3).cuda()
    es = (torch.randn(rows // nppf0, seg_enc, generator=g) * 3).cuda()
    x[0, 0], x[1, 1], x[2, 2] = 0.0, 65504.0 if dt == "f16" else 3e38, 1e-7
    hi, lo, seg = _expected_restore(x, es, nppf0, t16(dt))
    seg0 = d_obj - seg_enc
    FILL16, FILL32 = 0x1234, -7.0
    y16 = torch.full((rows, ldc), FILL16, dtype=torch.int16, device="cuda")
    ylo = torch.full((rows, ldc), FILL16, dtype=torch.int16, device="cuda")
    ps = torch.full((rows, ldc), FILL32, device="cuda")
    x0, es0 = x.clone(), es.clone()
    a = L.ObjrestoreArgs()
    a.x, a.enc_seg, a.y16, a.y16_lo, a.prop_seg = (t.data_ptr() for t in (x, es, y16, ylo, ps))
    a.ldc, a.y16_dtype, a.n_rows, a.nppf0, a.d_obj, a.seg_enc = ldc, L.DTYPE[dt], rows, nppf0, d_obj, seg_enc
    L.check(L.load().vog_obj_restore(C.byref(a), L.stream_ptr()), "vog_obj_restore")
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(es, es0)
    assert torch.equal(y16[:, :d_obj], hi) and torch.equal(ylo[:, :d_obj], lo) and torch.equal(ps[:, seg0:d_obj], seg)
    assert bool((y16[:, d_obj:] == FILL16).all()) and bool((ylo[:, d_obj:] == FILL16).all())
    assert bool((ps[:, d_obj:] == FILL32).all()) and bool((ps[:, :seg0] == FILL32).all())      # the proposal columns are not its to write
    assert bool((lo != 0).any()) and int(hi[0, 0]) == 0
    if dt == "f16":
        sub = hi[2, 2].view(torch.float16)
        assert 0 < float(sub) < 6.2e-5                                  # below the smallest normal f16
    # optional outputs: off the split plan there are no lo rows, without the sep head no segment part
    y16.fill_(FILL16), ylo.fill_(FILL16), ps.fill_(FILL32)
    a.y16_lo = None
    L.check(L.load().vog_obj_restore(C.byref(a), L.stream_ptr()), "vog_obj_restore")
    torch.cuda.synchronize()
    assert torch.equal(y16[:, :d_obj], hi) and bool((ylo == FILL16).all()) and torch.equal(ps[:, seg0:d_obj], seg)
    y16.fill_(FILL16), ps.fill_(FILL32)
    a.y16_lo, a.prop_seg, a.enc_seg = ylo.data_ptr(), None, None
    L.check(L.load().vog_obj_restore(C.byref(a), L.stream_ptr()), "vog_obj_restore")
    torch.cuda.synchronize()
    assert torch.equal(y16[:, :d_obj], hi) and torch.equal(ylo[:, :d_obj], lo) and bool((ps == FILL32).all())
    # the segment part alone (a model without mul_tx: nobody reads a 16-bit copy)
    y16.fill_(FILL16), ylo.fill_(FILL16)
    a.y16, a.y16_lo, a.prop_seg, a.enc_seg = None, None, ps.data_ptr(), es.data_ptr()
    L.check(L.load().vog_obj_restore(C.byref(a), L.stream_ptr()), "vog_obj_restore")
    torch.cuda.synchronize()
    assert torch.equal(ps[:, seg0:d_obj], seg) and bool((ps[:, :seg0] == FILL32).all()) and bool((y16 == FILL16).all()) and bool((ylo == FILL16).all())


# ---- 2: the rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_CASES)
def test_obj_rows_and_restored_stages_equal_the_raw_forward(name):
    """vog_ctx_obj_videos returns the bits the raw forward's last obj_tx layer wrote; after a cached forward into a workspace
    pre-filled with 0xA5 the 16-bit copy (models with mul_tx), its remainder (hi + lo plan) and the segment columns of prop_seg
    hold the raw forward's bits - and the proposal columns of prop_seg and obj_tx's own fp32 stage were not written at all."""
    eng, cfg, sd, batch, c, dev = build_engine(name, cached=True)
    T = int(batch["srl_arg_word_mask_len"].max())
    d = eng.desc
    assert (eng.plan == "split") == (name == SHARP16)
    has_mul = cfg.mdl.name == "vog"
    last = _last(eng)
    obj = _objed(eng, dev)
    eng.forward(dev, T=T)
    torch.cuda.synchronize()
    want32 = _stage(eng, dev, T, last, torch.float32).clone()
    assert torch.equal(obj[OBJ[0]].reshape(want32.shape), want32) and want32.abs().sum() > 0
    names = ([last + "16"] if has_mul else []) + ([last + "16_lo"] if has_mul and eng.plan == "split" else [])
    want = {n: _stage(eng, dev, T, n, torch.int16).clone() for n in names}
    want_ps = _stage(eng, dev, T, "prop_seg", torch.float32).clone()
    assert torch.equal(obj[OBJ[1]].reshape(-1, d.seg_enc).repeat_interleave(d.nppf0, dim=0), want_ps[:, d.prop_enc:])
    B, ncmp = eng._geometry(dev)[:2]
    for n in names + ["prop_seg", last]:                      # (the cached run has to write them, not inherit them)
        eng.stage(B, ncmp, T, n, torch.uint8, (want32.numel() * (2 if n in names else 4),)).fill_(0xA5)
    eng.forward(obj, T=T)
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(_stage(eng, dev, T, n, torch.int16), want[n]), (name, n)
    if name == SHARP16:
        assert len(names) == 2 and bool((want[last + "16_lo"] != 0).any())
    got_ps = _stage(eng, dev, T, "prop_seg", torch.float32)
    assert torch.equal(got_ps[:, d.prop_enc:], want_ps[:, d.prop_enc:]), name
    a5 = torch.full((1,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
    assert bool((got_ps[:, :d.prop_enc].contiguous().view(torch.int32) == a5).all())
    assert bool((_stage(eng, dev, T, last, torch.float32).view(torch.int32) == a5).all())       # read in place, never copied


# ---- 3: the whole forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_CASES + ["small/vog_sep_cmpmsk", "full/vog_sep_gt5_bs4_ragged"])
def test_whole_forward_equals_the_raw_path(name):
    """Every output from OBJ_KEYS == from raw inputs, eager and from a graph slot; the inputs are not modified; the cached
    outputs hold the bounds of tests/test_gpu_forward.py against the reference golden."""
    eng, cfg, sd, batch, c, dev = build_engine(name, cached=True)
    T = int(batch["srl_arg_word_mask_len"].max())
    obj = _objed(eng, dev)
    raw_out = eng.forward(dev, T=T)
    torch.cuda.synchronize()
    raw_out = {k: raw_out[k].clone() for k in OUT_KEYS}
    before = {k: v.clone() for k, v in obj.items()}
    out = eng.forward(obj, T=T)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert torch.equal(out[k], raw_out[k]), (name, k)
    slot = eng.make_slot(obj, T=T, graph=True)
    sout = slot.launch()
    torch.cuda.synchronize()
    slot.check()
    for k in OUT_KEYS:
        assert torch.equal(sout[k], raw_out[k]), (name, "slot", k)
    for k in before:
        assert torch.equal(before[k], obj[k]), k
    assert torch.isfinite(out["mdl_outs"]).all()
    ncmp = batch["new_srl_idxs"].shape[1]
    _check_against(name, out, eng.unpack_pred(out["pred_rec"], ncmp), np.load(cases.golden_path(name)), None, tol_rel=1e-3, tol_logit=6e-3)


# ---- 4: the launch trace -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small/vog_sep", "small/vgrnd_sep", CFG5, "full/vog_sep_gt5_bs4_ragged"])
def test_launch_trace_of_a_cached_batch(name):
    """One `obj_restore` in place of the feature cast, every encoder step and every obj_tx step; both BiLSTM layers launch alone,
    obj_restore directly behind the first; lstm_outproj + mul_pv keeps its partner; every other launch in the raw order. The raw
    trace of the same batch is what it was."""
    eng, cfg, sd, batch, c, dev = build_engine(name, cached=True)
    T = int(batch["srl_arg_word_mask_len"].max())
    raw = _trace(eng, dev, T)
    cached = _trace(eng, _objed(eng, dev), T)
    assert _trace(eng, dev, T) == raw
    fc, fr = _flat(cached), _flat(raw)
    gone = lambda p: p in ENCODER_STEPS or p in ("vis_concat", "vis_prep") or p.startswith("obj_")
    assert fc.count("obj_restore") == 1 and not [p for p in fc if gone(p) and p != "obj_restore"]
    assert set(fr) & set(ENCODER_STEPS) and [p for p in fr if p.startswith("obj_")] and "obj_restore" not in fr
    assert [p for p in fc if not gone(p)] == [p for p in fr if not gone(p)]
    i = fc.index("obj_restore")
    consumers = [p for p in fc if p in ("mul_pv", "vislang", "pred_cmp")]
    assert "pred_cmp" in consumers and len(consumers) >= 2 and all(fc.index(p) > i for p in consumers)
    if name.startswith("full/"):
        assert "lstm_layer+vis_enc" in raw and "lstm_layer+obj_tail" in raw and "lstm_outproj+mul_pv" in raw
        assert [n for n in cached if "+" in n] == ["lstm_outproj+mul_pv"]
        assert cached.count("lstm_layer") == 2 and cached[cached.index("lstm_layer") + 1] == "obj_restore"


# ---- 5: ObjBank ------------------------------------------------------------------------------------------------------------------
def _banks(eng, cfg, c, batch, nv=13, seed=17):
    """13 videos: full chunks of B * ncmp videos and a short last one, for every case that does not ask for another number."""
    raw = dls.FeatureBank(cfg, comm_for(c), nv, dtype="f32", n_gt=8)
    raw.put(0, _pool(nv, cfg, c, seed))
    Bq, ncmp = batch["num_cmp_msk"].shape
    assert nv != 13 or nv % (Bq * ncmp) != 0
    return raw, dls.ObjBank.encode(raw, eng, Bq, ncmp)


@pytest.mark.parametrize("name", ["small/vog_sep", "small/vog_svsq"])
def test_obj_bank_loader_and_fed_pipeline_equal_the_raw_bank(name):
    """Batches of `ObjBank.loader` against the raw bank's loader (random indices: a video sits at another batch position than the
    one it was encoded at), then the same through FedPipeline(..., assembler=bank)."""
    eng, cfg, sd, batch, c, dev = build_engine(name)
    T = int(batch["srl_arg_word_mask_len"].max())
    raw, bank = _banks(eng, cfg, c, batch)
    d = eng.desc
    Bq, ncmp = batch["num_cmp_msk"].shape
    assert isinstance(bank, dls.EncodedBank) and (bank.prop_dim, bank.seg_dim, bank.dtype) == (d.prop_enc + d.seg_enc, d.seg_enc, "f32")
    assert bank.nbytes == bank.V * dls.ObjBank.bytes_per_video(c["nppf0"], d.prop_enc, d.seg_enc, 8)
    assert (bank.epoch, bank.plan, bank.geometry) == (eng.weights_epoch, eng.plan, (Bq, ncmp))
    assert bank.lossless_for(eng) and bank.fwd_keys == ("pad_proposals",) + OBJ and bank.encode_seconds > 0
    with pytest.raises(TypeError):
        bank.put(0, {})
    ibs = _index_batches(batch, cfg, c, raw.V, 3)
    n = 0
    for rb, ob in zip(raw.loader(ibs), bank.loader(ibs)):
        assert set(rb) - set(FEATS) == set(ob) - set(OBJ) and set(FEATS) <= set(rb) and set(OBJ) <= set(ob) and not set(FEATS) & set(ob)
        for k in set(rb) - set(FEATS):                                  # loss keys, proposals, language: identical
            assert torch.equal(rb[k], ob[k]), k
        o_raw, o_obj = eng.forward(rb, T=T), eng.forward(ob, T=T)
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.equal(o_raw[k], o_obj[k]), (n, k)
        n += 1
    assert n == 3
    bank.check()
    # the same rows from host items, the raw features never a bank on the device
    pool = _pool(raw.V, cfg, c, 17)
    chunks = [(s0, {k: v[s0:s0 + 5] for k, v in pool.items()}) for s0 in range(0, raw.V, 5)]
    bank2 = dls.ObjBank.from_items(cfg, comm_for(c), raw.V, chunks, eng, Bq, ncmp, n_gt=8)
    for k in bank.tab:
        assert torch.equal(bank.tab[k], bank2.tab[k]), k
    with pytest.raises(L.VogError, match="raw bank"):
        bank2.refresh()
    # fed slots
    lang = {k: dev[k] for k in LANG_KEYS}
    ex = bank(torch.zeros(Bq, ncmp, dtype=torch.int32).cuda(), with_loss_keys=False)
    ex.pop("_keepalive")
    assert set(ex) == set(bank.fwd_keys)
    ex.update(lang)
    spec = {"vid_index": np.zeros((Bq, ncmp), np.int32), **{k: np.zeros_like(batch[k]) for k in LANG_KEYS}}
    pipe = engine_mod.FedPipeline(eng, ex, spec, assembler=bank, streams=2, slots_per_stream=2, T=T)
    assert set(pipe.slots[0].fed_keys) == set(bank.fwd_keys) | set(LANG_KEYS)
    with pytest.raises(ValueError, match="other feature keys"):        # a raw bank cannot feed a slot made from cached rows
        eng.make_slot(ex, T=T, graph=True).feed_from(dls.PackedStaging(spec, n_dev=1), assembler=raw, via="device")
    rng = np.random.default_rng(21)
    first = None
    for i in range(4):
        idx = rng.integers(0, raw.V, size=(Bq, ncmp)).astype(np.int32)
        st = pipe.next_staging()
        st.fill({"vid_index": idx})
        st.fill({k: batch[k] for k in LANG_KEYS})
        sl = pipe.submit()
        pipe.done(sl).synchronize()
        got = {k: sl.out[k].clone() for k in OUT_KEYS}
        r_in = raw(torch.from_numpy(idx).cuda(), with_loss_keys=False)
        o_raw = eng.forward({**lang, **{k: r_in[k] for k in raw.fwd_keys}}, T=T)
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.equal(got[k], o_raw[k]), (i, k)
        first = first if first is not None else got
    assert not torch.equal(first["mdl_outs"], got["mdl_outs"])
    for sl in pipe.slots:
        sl.check()


@pytest.mark.parametrize("name", ["small/vog_sep", "small/vog_svsq"])
def test_evaluator_on_an_obj_bank_equals_the_raw_bank(name, tmp_path, tmp_path_factory):
    """Evaluator.forward with val_graph, device metrics and the pickle on `bank.loader(index_batches)`: the loss dict, the metric
    dict and the pickle bytes of the raw bank's run - through the fed slots' epilogue, with and without the query bank, and
    through the existing loop. Six batches of 4, the last a query short: the tail batch takes the eager calls at B = 3 with rows
    made for B = 4."""
    from tests import test_gpu_device_metrics as T
    from tests.test_gpu_val_graph import _run
    cfg, sd, comm, sel, dl = T.make_eval_set(name, tmp_path_factory.mktemp("ann_obj_" + name.replace("/", "_")), n_batches=6, B=4, distinct=5)
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
    bank = dls.ObjBank.encode(raw, mdl.engine(), *dl[0]["num_cmp_msk"].shape)
    ref = _run(cfg, mdl, evl, loss_fn, raw.loader(ibs), tmp_path / "raw", device_metrics=True, val_graph=True)
    assert ref[3] == "graph" and ref[0]["loss"] > 0 and ref[2] is not None and len(pickle.loads(ref[2])) == sum(len(b["sent_idx"]) for b in ibs)
    for tag, hip in (("graph", {"val_graph": True}), ("queries", {"val_graph": True, "query_bank": True}), ("eager", {})):
        got = _run(cfg, mdl, evl, loss_fn, bank.loader(ibs), tmp_path / tag, device_metrics=True, **hip)
        cfg.hip["query_bank"] = False
        assert got[3] == ("eager" if tag == "eager" else "graph"), tag
        assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2], (tag, got[0], ref[0], got[1], ref[1])
    bank.check()


def test_obj_bank_guards_a_bad_index():
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_sep", cached=True)
    raw, bank = _banks(eng, cfg, c, batch)
    Bq, ncmp = batch["num_cmp_msk"].shape
    idx = np.random.default_rng(5).integers(0, raw.V, size=(Bq, ncmp)).astype(np.int32)
    good = bank(torch.from_numpy(idx).cuda(), with_loss_keys=False)
    idx[1, 2] = raw.V
    with pytest.raises(ValueError, match="outside"):
        bank(torch.from_numpy(idx), with_loss_keys=False)
    got = bank(torch.from_numpy(idx).cuda(), with_loss_keys=False)
    torch.cuda.synchronize()
    assert not got[OBJ[0]][1, 2].any() and not got[OBJ[1]][1, 2].any() and bool(good[OBJ[0]][1, 2].any())
    keep = torch.ones(Bq, ncmp, dtype=torch.bool)
    keep[1, 2] = False
    assert torch.equal(got[OBJ[0]][keep], good[OBJ[0]][keep])
    with pytest.raises(L.VogError, match="outside"):
        bank.check()
    bank.check()                                                       # reported once


def test_obj_bank_goes_stale_with_the_weights_and_refreshes():
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_sep")
    T = int(batch["srl_arg_word_mask_len"].max())
    raw, bank = _banks(eng, cfg, c, batch)
    ibs = _index_batches(batch, cfg, c, raw.V, 1)
    old = bank.tab["pad_region_feature"].clone()
    sd2 = dict(sd)
    rng = np.random.default_rng(9)
    for k in ("obj_txf.encoder.layers.0.selfattn.layer.wv.weight", "obj_txf.encoder.layers.0.feedforward.layer.linear2.bias"):
        sd2[k] = (sd[k] + 0.05 * rng.standard_normal(sd[k].shape)).astype(np.float32)       # (obj_tx alone: the encoders' rows stay)
    eng.load_state_dict(sd2)
    assert bank.stale() and not bank.lossless_for(eng)
    with pytest.raises(L.VogError, match="refresh"):
        bank.check()
    with pytest.raises(L.VogError, match="refresh"):                   # (stale until refreshed: not a once-only report)
        next(iter(bank.loader(ibs))), bank.check()
    assert bank.refresh() is bank and not bank.stale() and bank.epoch == eng.weights_epoch
    assert not torch.equal(old, bank.tab["pad_region_feature"])
    bank.check()
    rb, ob = next(iter(raw.loader(ibs))), next(iter(bank.loader(ibs)))
    o_raw, o_obj = eng.forward(rb, T=T), eng.forward(ob, T=T)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert torch.equal(o_raw[k], o_obj[k]), k


# ---- 6: plan changes and the logit guard -------------------------------------------------------------------------------------
def _covering_batches(raw, batch, cfg, c):
    """Index batches that name every video of the bank, chunk by chunk as `encode` walks them (the short last chunk filled up
    with its first video)."""
    Bq, ncmp = batch["num_cmp_msk"].shape
    per = Bq * ncmp
    ibs = _index_batches(batch, cfg, c, raw.V, (raw.V + per - 1) // per)
    for i, ib in enumerate(ibs):
        ids = np.arange(i * per, (i + 1) * per)
        ids[ids >= raw.V] = i * per
        ib["vid_index"] = torch.from_numpy(ids.astype(np.int32).reshape(Bq, ncmp))
    return ibs


def test_encode_reports_the_logits_obj_tx_saw():
    """After ObjBank.encode alone - not one forward - observed_logit_max()[0] is what a fresh engine reports after raw forwards
    over the same videos; mul_tx has not run, its word is 0."""
    eng, cfg, sd, batch, c, dev = build_engine(SHARP16)
    assert eng.plan == "split" and eng.observed_logit_max() == (0.0, 0.0)
    raw, bank = _banks(eng, cfg, c, batch)
    seen = eng.observed_logit_max()
    assert seen[0] > 0 and seen[1] == 0.0 and not bank.stale() and eng.plan == "split"
    e2, *_ = build_engine(SHARP16)
    T = int(batch["srl_arg_word_mask_len"].max())
    for rb in raw.loader(_covering_batches(raw, batch, cfg, c)):
        e2.forward(rb, T=T)
    torch.cuda.synchronize()
    assert e2.observed_logit_max()[0] == seen[0], (e2.observed_logit_max(), seen)
    assert e2.observed_logit_max()[1] > 0


def test_plan_change_makes_the_bank_stale_and_a_raised_plan_is_re_encoded(monkeypatch):
    """full/vog_sep_sharp8 plans f16; one query of it is 4 videos = 200 rows, inside one band of the fused tail on either plan.
    (a) The plan moved by a reload under `split`: stale, an error until `refresh`, then the rows are the split plan's.
    (b) The guard: with the f16 logit limit lowered under what obj_tx reports, `encode` itself raises the plan
    (check_logit_scale behind its synchronisation) and encodes once more - the bank comes back fresh, on `split`, and its
    batches equal the raw path's."""
    name = "full/vog_sep_sharp8"
    eng, cfg, sd, batch, c, dev = build_engine(name)
    batch = {k: np.ascontiguousarray(v[:1]) for k, v in batch.items()}
    T = int(batch["srl_arg_word_mask_len"].max())
    assert eng.plan == "f16" and eng.obj_band_rows() == 512
    raw, bank = _banks(eng, cfg, c, batch)
    assert bank.plan == "f16" and not bank.stale() and bank.geometry == (1, 4) and bank.lossless_for(eng)
    ibs = _index_batches(batch, cfg, c, raw.V, 1)

    def same_as_raw(e, bk):
        rb, ob = next(iter(raw.loader(ibs))), next(iter(bk.loader(ibs)))
        o_raw, o_obj = e.forward(rb, T=T), e.forward(ob, T=T)
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.equal(o_raw[k], o_obj[k]), k
    same_as_raw(eng, bank)
    f16_rows = bank.tab["pad_region_feature"].clone()
    eng.tx_request = "split"
    eng.load_state_dict(sd)
    assert eng.plan == "split" and bank.stale() and not bank.lossless_for(eng) and eng.obj_band_rows() == 256
    with pytest.raises(L.VogError, match="refresh"):
        bank.check()
    assert not bank.refresh().stale() and bank.plan == "split" and bank.lossless_for(eng)
    assert not torch.equal(f16_rows, bank.tab["pad_region_feature"])
    same_as_raw(eng, bank)
    # (b)
    e2, *_ = build_engine(name)
    assert e2.plan == "f16"
    monkeypatch.setattr(engine_mod, "F16_LOGIT_MAX", 1e-3)
    with pytest.warns(UserWarning, match="re-planning"):
        bank2 = dls.ObjBank.encode(raw, e2, *batch["num_cmp_msk"].shape)
    assert e2.plan == "split" and bank2.plan == "split" and not bank2.stale() and bank2.epoch == e2.weights_epoch
    assert torch.equal(bank2.tab["pad_region_feature"], bank.tab["pad_region_feature"])
    same_as_raw(e2, bank2)


def test_rows_carry_the_tail_band_they_were_made_in():
    """The limit of the bit-equality, pinned: the fused tail's fp32 summation order is that of the band of 8 row blocks a row
    lies in (512 rows at f16). Four queries of full/vog_sep_gt5_bs4_ragged are 800 rows: a video used in the band it was made in
    keeps the raw path's bits, a video that crosses the boundary does not - the bank says so (`lossless_for`), and the outputs
    stay inside twice the bound each path holds against the fp32 reference (tests/test_gpu_forward.py: 6e-3 on the logits).
    Where the tail runs as separate launches (the small models) there are no bands."""
    small, *_ = build_engine("small/vog_sep", cached=True)
    assert small.obj_band_rows() == 0
    eng, cfg, sd, batch, c, dev = build_engine("full/vog_sep_gt5_bs4_ragged", cached=True)
    T = int(batch["srl_arg_word_mask_len"].max())
    assert eng.plan == "f16" and eng.obj_band_rows() == 512
    raw, bank = _banks(eng, cfg, c, batch, nv=16)
    assert bank.geometry == (4, 4) and not bank.stale() and not bank.lossless_for(eng)
    ib = _index_batches(batch, cfg, c, raw.V, 1)[0]
    outs = {}
    for tag, ids in (("same band", [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 10, 12, 11, 14, 13, 15]), ("crossed", list(range(15, -1, -1)))):
        ib["vid_index"] = torch.tensor(ids, dtype=torch.int32).reshape(4, 4)
        rb, ob = next(iter(raw.loader([ib]))), next(iter(bank.loader([ib])))
        o_raw, o_obj = eng.forward(rb, T=T), eng.forward(ob, T=T)
        torch.cuda.synchronize()
        outs[tag] = float((o_raw["mdl_outs"] - o_obj["mdl_outs"]).abs().max())
        print(tag, "max |mdl_outs difference|", outs[tag])
    assert outs["same band"] == 0.0 and 0.0 < outs["crossed"] <= 1.2e-2


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_restriction(tmp_path):
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_sep", cached=True)
    obj = _objed(eng, dev)
    d = eng.desc
    with pytest.raises(ValueError, match="make_batched takes raw features"):
        eng.make_batched([obj, obj])
    with pytest.raises(ValueError, match="make_group takes raw features"):
        eng.make_group([obj, obj])
    with pytest.raises(ValueError, match="pair"):                      # obj_out without enc_seg
        eng.forward({k: v for k, v in obj.items() if k != OBJ[1]})
    with pytest.raises(ValueError, match="never a mix"):               # next to raw features
        eng.forward({**obj, FEATS[0]: dev[FEATS[0]]})
    with pytest.raises(ValueError, match="never a mix"):
        eng.forward({**obj, ENC[0]: obj[OBJ[0]][..., :d.prop_enc].contiguous()})
    with pytest.raises(ValueError, match="expected"):
        eng.forward({**obj, OBJ[0]: obj[OBJ[0]][..., :d.prop_enc].contiguous()})
    with pytest.raises(ValueError, match="float32 tensor on the device"):
        eng.forward({**obj, OBJ[0]: obj[OBJ[0]].cpu()})
    # the C entry says the same before anything is launched
    b, _, (B, ncmp, T) = eng.make_batch(obj)
    b.enc_seg = None
    with pytest.raises(L.VogError, match="obj_out comes with enc_seg"):
        eng.describe_steps(b, eng.workspace(B, ncmp, T))
    # engines whose obj_tx is not per video, or that have none
    for other in ("small/vog_spat", "small/vog_temp", "small/igrnd_sep"):
        eo, cfo, _, bo, co, devo = build_engine(other, cached=True)
        Bo, no = bo["num_cmp_msk"].shape
        do = eo.desc
        NPv = do.nfrm0 * do.nppf0
        args = (devo[FEATS[0]].reshape(Bo * no, NPv, -1), devo[FEATS[1]].reshape(Bo * no, do.nfrm0, -1), devo["pad_proposals"].reshape(Bo * no, NPv, 7))
        with pytest.raises(L.VogError, match="EncodedBank already covers"):
            eo.obj_videos(*args, Bo, no)
        with pytest.raises(ValueError, match="EncodedBank already covers"):
            dls.ObjBank(cfo, comm_for(co), 4)
        fake = {k: v for k, v in devo.items() if k not in FEATS}
        lead = devo[FEATS[0]].shape[:-2]
        fake[OBJ[0]] = torch.zeros(lead + (devo[FEATS[0]].shape[-2], do.prop_enc + do.seg_enc), device="cuda")
        fake[OBJ[1]] = torch.zeros(lead + (devo[FEATS[1]].shape[-2], do.seg_enc), device="cuda")
        with pytest.raises(L.VogError, match="EncodedBank already covers"):
            eo.forward(fake)
    # the fp32 plan reads raw features
    e32, *_ = build_engine("small/vog_sep", tx_dtype="f32", cached=True)
    assert e32.precise is not None and e32.plan == "f32"
    with pytest.raises(L.VogError, match="fp32 path reads raw features"):
        e32.forward(obj)
    with pytest.raises(L.VogError, match="fp32 path reads raw features"):
        e32.make_slot(obj)
    with pytest.raises(L.VogError, match="fp32 path reads raw features"):
        _objed(e32, dev)
    # ... also when the plan is raised at run time: the observed logit scale escalates `auto` before the batch is read
    e2, *_ = build_engine("small/vog_sep")
    e2._stats[:2] = torch.tensor([1e9, 1e9]).view(torch.int32)
    with pytest.warns(UserWarning):
        with pytest.raises(L.VogError, match="fp32 path reads raw features"):
            e2.forward(obj)
    assert e2.plan == "f32"
    # training: obj_tx is being trained
    tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
    sel = importlib.import_module("vognet-pytorch_amd.mdl_selector").get_mdl_loss_eval(cfg)
    comm = comm_for(c)
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    raw, bank = _banks(eng, cfg, c, batch)
    ibs = _index_batches(batch, cfg, c, raw.V, 1)
    learn = tu.Learner(uid="obj", data=tu.DataWrap(path=tmp_path, train_dl=bank.loader(ibs), valid_dl=bank.loader(ibs)), mdl=mdl,
                       loss_fn=sel["loss"](cfg, comm), cfg=cfg, eval_fn=sel["eval"](cfg, comm, torch.device("cuda", 0)), comm=comm)
    ob = next(iter(bank.loader(ibs)))
    with pytest.raises(L.VogError, match="trains the encoders and obj_tx"):
        learn.trainer.step(ob)
    with pytest.raises(L.VogError, match="trains the encoders and obj_tx"):
        learn.train_epoch()
    assert learn.trainer.num_it == 0


def test_main_dist_feature_bank_obj(capsys, tmp_path):
    """`main_dist --only_val --feature_bank=obj` on svsq (full-size VOGNet, a short tail batch) prints the loss and the metrics of
    `--feature_bank=f16` and leaves the same pickle bytes; on spat it refuses with the rule as the exit text."""
    import json
    main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
    over = {"mdl.name": "vog", "ds.conc_type": "svsq", "mdl.obj_tx.use_rel": True, "mdl.mul_tx.use_rel": True, "train.bsv": 4}
    res = {}
    for kind in ("f16", "obj"):
        main_mod.main_dist("v_" + kind, only_val=True, synthetic_batches=3, feature_bank=kind, feature_bank_videos=32,
                           **over, **{"misc.tmp_path": str(tmp_path / kind)})
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{\"uid\"")][-1]
        res[kind] = (json.loads(line), open(tmp_path / kind / "predictions" / ("v_" + kind) / "valid_0.pkl", "rb").read())
    assert res["obj"][0]["feature_bank"] == "obj" and res["obj"][0]["queries"] == 11
    assert res["obj"][0]["val_loss"] == res["f16"][0]["val_loss"] and res["obj"][0]["val_acc"] == res["f16"][0]["val_acc"]
    assert res["obj"][1] == res["f16"][1] and len(pickle.loads(res["obj"][1])) == 11
    with pytest.raises(SystemExit, match="EncodedBank already covers"):
        main_mod.main_dist("v_spat", only_val=True, feature_bank="obj", **{**over, "ds.conc_type": "spat"},
                           **{"misc.tmp_path": str(tmp_path / "bad")})
