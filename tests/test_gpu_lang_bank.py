"""-m gpu: forwards from the language chain's results (vog_batch.shared_lang / shared_final_hidden -> the engine's vector form,
`ARG_KEYS`) and the language bank (dat_loader_simple.LangBank, filled through `VogEngine.encode_queries` -> vog_lang_forward).

The rows are the bits vog_lang_forward computes for a pseudo-batch; a vector-form forward is, bit for bit, the member of a
one-member group (`make_group([inp], graph=False)`: the same language launches, the same member launches) - eager and from a
graph slot; against the stand-alone word-form forward it holds the group test's bound (1.5e-3 abs on mdl_outs, 4e-4 on the
prediction scores: tests/test_gpu_forward.py::test_group_language_encoder_matches_standalone_forwards) and against the reference
goldens the tolerances of `_check_against`. `bank_prep` (one launch for mul_pl + vis_prep + vis_concat / obj_restore) leaves
the same bits as the three launches."""
import ctypes as C
import importlib
import json
import pickle

import numpy as np
import pytest
import torch

from oracle import cases
from tests import test_gpu_device_metrics as TDM
from tests.gpu_util import L, build_engine, comm_for, engine_mod
from tests.gpu_util import encoded as _encoded, objed as _obj_rows, trace as _trace, video_pool as _pool
from tests.test_gpu_forward import _check_against
from tests.test_gpu_val_graph import _eval_set, _run

pytestmark = pytest.mark.gpu

dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
synth = importlib.import_module("vognet-pytorch_amd.synth")

ARG = engine_mod.ARG_KEYS
WORDS = engine_mod.WORD_KEYS
LANG5 = engine_mod.LANG_KEYS
FEATS = ("pad_region_feature", "seg_feature_for_frms")
OUT_KEYS = ("mdl_outs", "mdl_outs_eval", "pred_rec")
SEP_KEYS = ("vidf_outs", "fin_scores_loss", "fin_scores")
CFG2 = "full/cfg2_vog_spat_gt5_bs4"
CFG5 = "full/cfg5_vog_svsq_gt5_bs16"
SEP_FULL = "full/vog_sep_gt5_bs4_ragged"
LOGIT_BOUND, SCORE_BOUND = 1.5e-3, 4e-4          # the group test's bound against the stand-alone word-form forward


def _vec(eng, dev, T):
    """The batch in vector form: the word-level keys replaced by encode_queries at the batch's own (B, T)."""
    B = int(dev["num_cmp_msk"].shape[0])
    lang, fh = eng.encode_queries({k: dev[k] for k in LANG5}, B, T)
    v = {k: t for k, t in dev.items() if k not in WORDS}
    v[ARG[0]] = lang
    if eng.sep:
        v[ARG[1]] = fh
    return v


def _lang_forward(eng, chunk, B, T):
    """vog_lang_forward on one pseudo-batch through the C interface, on a language workspace of the test's own: (lang, fh)."""
    d, lib = eng.desc, eng.lib
    nvl = int(chunk["srl_arg_words_ind"].shape[1])
    n = lib.vog_lang_workspace_bytes(eng.ctx, B, nvl, T)
    assert n > 0
    ws = torch.empty(int(n), dtype=torch.uint8, device="cuda")
    L.check(lib.vog_lang_workspace_init(eng.ctx, B, nvl, T, ws.data_ptr(), ws.numel(), L.stream_ptr()), "init")
    lb = L.Batch()
    lb.B, lb.ncmp, lb.T = B, nvl, T
    fault = torch.zeros(16, dtype=torch.int32).pin_memory()
    lb.fault = fault.data_ptr()
    keep = {k: chunk[k].contiguous() for k in LANG5}
    for k in LANG5:
        setattr(lb, k, L.ptr(keep[k]))
    L.check(lib.vog_lang_forward(eng.ctx, C.byref(lb), ws.data_ptr(), ws.numel(), L.stream_ptr()), "vog_lang_forward")
    lang, fh = C.c_void_p(), C.c_void_p()
    L.check(lib.vog_lang_outputs(eng.ctx, B, nvl, T, ws.data_ptr(), C.byref(lang), C.byref(fh)), "outputs")
    torch.cuda.synchronize()
    assert int(fault[0]) == 0
    o1, o2 = lang.value - ws.data_ptr(), fh.value - ws.data_ptr()
    a = ws[o1:o1 + 4 * B * nvl * d.nsrl * d.lang_enc].view(torch.float32).view(B, nvl, d.nsrl, d.lang_enc).clone()
    f = ws[o2:o2 + 4 * B * nvl * d.lang_enc].view(torch.float32).view(B, nvl, d.lang_enc).clone()
    return a, f


def _query_rows(batch, n):
    """n queries: the batch's rows in turn (row i = query i % B), so that a query's place inside its pseudo-batch varies."""
    B = batch["num_cmp_msk"].shape[0]
    idx = np.arange(n) % B
    keys = [k for k in batch if k not in FEATS + ("pad_proposals",)]
    return {k: torch.from_numpy(np.ascontiguousarray(batch[k][idx])) for k in keys}


# ---- 1: the rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep", "small/edge_temp_len1", "small/edge_sep_maxlen",
                                  "small/edge_spat_mixed_args"])
def test_lang_bank_rows_equal_vog_lang_forward(name):
    """13 queries at B = 4: three full pseudo-batches and a last one of one query filled up with its first. Every row of the
    bank equals, bit for bit, the row vog_lang_forward leaves for the same pseudo-batch; masked arguments give zero rows; the
    size is bytes_per_query; the other columns and the host columns are the query bank's."""
    eng, cfg, sd, batch, c, dev = build_engine(name, cached=True)
    d = eng.desc
    Q, B = 13, 4
    T = int(batch["srl_arg_word_mask_len"].max())
    rows = _query_rows(batch, Q)
    qb = dls.QueryBank.from_batches([rows], host_keys=["new_srl_idxs"])
    lbk = dls.LangBank.encode(qb, eng, B, T)
    torch.cuda.synchronize()
    nvl = int(rows["srl_arg_words_ind"].shape[1])
    assert nvl == (batch["num_cmp_msk"].shape[1] if eng.sep else 1)
    assert set(lbk.keys) == (set(qb.keys) - set(WORDS)) | set(ARG[:2 if eng.sep else 1])
    assert tuple(lbk.tab[ARG[0]].shape) == (Q, nvl, d.nsrl, d.lang_enc) and lbk.tab[ARG[0]].dtype == torch.float32
    per = dls.LangBank.bytes_per_query(d.nsrl, d.lang_enc, nvl, eng.sep)
    assert per == 4 * nvl * d.lang_enc * (d.nsrl + (1 if eng.sep else 0))
    assert sum(lbk.row_bytes(k) for k in ARG if k in lbk.tab) == per
    assert lbk.geometry == (B, T) and lbk.lossless_for(eng) and not lbk.stale() and lbk.encode_seconds > 0
    for k in lbk.keys:
        if k not in ARG:
            assert torch.equal(lbk.tab[k], qb.tab[k]), k
    assert np.array_equal(lbk.meta(np.arange(Q))["new_srl_idxs"], rows["new_srl_idxs"].numpy())
    src = {k: qb.tab[k] for k in LANG5}
    for s0 in range(0, Q, B):
        chunk = {k: v[s0:s0 + B] for k, v in src.items()}
        m = int(chunk["srl_arg_words_ind"].shape[0])
        if m < B:
            chunk = {k: torch.cat([v, v[:1].expand((B - m,) + tuple(v.shape[1:]))]) for k, v in chunk.items()}
        a, f = _lang_forward(eng, chunk, B, T)
        assert torch.equal(lbk.tab[ARG[0]][s0:s0 + m], a[:m]), (name, s0)
        if eng.sep:
            assert torch.equal(lbk.tab[ARG[1]][s0:s0 + m], f[:m]), (name, s0)
    assert m == 1                                                   # (the filled last chunk was exercised)
    msk = qb.tab["srl_arg_inds_msk"] != 0
    vec = lbk.tab[ARG[0]]
    assert torch.isfinite(vec).all() and bool((vec[msk].abs().sum(-1) > 0).all())
    assert not bool(vec[~msk].any())                                # masked arguments: zero rows
    if name == "small/edge_spat_mixed_args":
        assert bool((~msk).any()) and bool(msk.any())
    with pytest.raises(TypeError, match="encode / refresh"):
        lbk.put(0, {ARG[0]: vec[:1]})
    with pytest.raises(ValueError, match="word-level"):
        dls.LangBank.encode(lbk, eng, B, T)


# ---- 2: the whole forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "small/vog_sep", "small/igrnd_spat", CFG2])
def test_vector_form_forward_equals_the_group_member(name):
    """Vector-form batch with raw features: eager `forward` and a graph slot equal the member of a one-member group bit for
    bit on every output and the prediction records, and each other; against the stand-alone word-form forward the group test's
    bound; against the reference golden `_check_against`'s tolerances. The same batch with encoder outputs in place of the raw
    features (EncodedBank rows at the bound (B, T)) is compared with the stand-alone forward as well: measured and printed,
    held to the bound (the result is recorded in LangBank.lossless_for)."""
    eng, cfg, sd, batch, c, dev = build_engine(name, cached=True)
    T = int(batch["srl_arg_word_mask_len"].max())
    ncmp = batch["new_srl_idxs"].shape[1]
    keys = OUT_KEYS + (SEP_KEYS if eng.sep else ())
    alone = eng.forward(dev, T=T)
    torch.cuda.synchronize()
    alone = {k: alone[k].clone() for k in keys}
    grp = eng.make_group([dev], graph=False)
    gout = grp.launch()[0]
    torch.cuda.synchronize()
    member = {k: gout[k].clone() for k in keys}
    vec = _vec(eng, dev, T)
    assert engine_mod.language_kind(vec) == "vec" and engine_mod.language_kind(dev) == "words"
    before = {k: v.clone() for k, v in vec.items()}
    b, _, _ = eng.make_batch(vec, T)
    assert b.shared_lang == vec[ARG[0]].data_ptr() and not b.srl_arg_words_ind and not b.srl_arg_word_mask_len and not b.fault
    assert bool(b.shared_final_hidden) == eng.sep
    out = eng.forward(vec, T=T)
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(out[k], member[k]), (name, "eager vs group member", k)
    slot = eng.make_slot(vec, T=T, graph=True)
    for rep in range(2):
        slot.out["mdl_outs"].fill_(float("nan"))
        sout = slot.launch()
        torch.cuda.synchronize()
        slot.check()
        for k in keys:
            assert torch.equal(sout[k], member[k]), (name, "replay vs group member", rep, k)
    for k in before:
        assert torch.equal(before[k], vec[k]), k                       # inputs are never modified
    # T is the caller's or 1: no host read of lengths that are not there, and the results do not depend on it
    out1 = eng.forward(vec)
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(out1[k], member[k]), (name, "T = 1", k)
    # the stand-alone word-form forward: the group test's bound
    e = (out["mdl_outs"] - alone["mdl_outs"]).abs().max().item()
    pa, pb = eng.unpack_pred(alone["pred_rec"], ncmp), eng.unpack_pred(out["pred_rec"], ncmp)
    es = (pa["scores"] - pb["scores"]).abs().max().item()
    print(name, "vector form vs stand-alone: logits", e, "scores", es, "bit-equal", all(torch.equal(out[k], alone[k]) for k in keys))
    assert e <= LOGIT_BOUND and es <= SCORE_BOUND, (name, e, es)
    _check_against(name, out, pb, np.load(cases.golden_path(name)), None, tol_rel=1e-3, tol_logit=6e-3)
    # ... and with EncodedBank rows at the bound (B, T)
    if eng.precise is None:
        ve = {k: v for k, v in _encoded(eng, dev).items() if k not in WORDS}
        ve.update({k: vec[k] for k in ARG if k in vec})
        oe = eng.forward(ve, T=T)
        torch.cuda.synchronize()
        print(name, "vector form + encoded rows vs stand-alone: bit-equal", all(torch.equal(oe[k], alone[k]) for k in keys),
              "logits", (oe["mdl_outs"] - alone["mdl_outs"]).abs().max().item())
        assert (oe["mdl_outs"] - alone["mdl_outs"]).abs().max().item() <= LOGIT_BOUND


# ---- 3: the prologue --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,nq", [(CFG2, "enc", None), (CFG5, "obj", None), (SEP_FULL, "obj", 2), ("small/vog_spat", "enc", None)])
def test_bank_prep_is_one_launch_with_the_same_bits(name, rows, nq):
    """A vector-form batch whose visual rows are banked: with pair_launches the prologue is ONE launch, `bank_prep`, wherever
    the rule holds - structured mul_tx layer 0 and M = Bn * nsrl <= 64 rows (cfg 2: 20 rows; the first two queries of the full sep
    case: 40 rows, the obj_restore form) - and the three launches where it does not (cfg 5: 16 sentences x 5 arguments = 80 rows;
    the small model: mul_tx's layer 0 is not structured); with pair_launches = 0 always the three. Outputs of the two are
    bit-equal. With raw features the vector-form trace is the group member's, as before."""
    eng, cfg, sd, batch, c, dev = build_engine(name, cached=True)
    if nq is not None:
        dev = {k: v[:nq].contiguous() for k, v in dev.items()}
    T = int(dev["srl_arg_word_mask_len"].max())
    d = eng.desc
    vec = _vec(eng, dev, T)
    banked = {k: v for k, v in (_encoded(eng, dev) if rows == "enc" else _obj_rows(eng, dev)).items() if k not in WORDS}
    banked.update({k: vec[k] for k in ARG if k in vec})
    keys = OUT_KEYS + (SEP_KEYS if eng.sep else ())
    three = ["mul_pl", "vis_prep", "vis_concat" if rows == "enc" else "obj_restore"]
    Bn = eng._geometry(dev)[0] * eng._geometry(dev)[2]
    structured = name.startswith("full/")
    fused = structured and Bn * d.nsrl <= 64
    assert fused == (name in (CFG2, SEP_FULL))
    on = _trace(eng, banked, T)
    o_on = eng.forward(banked, T=T)
    torch.cuda.synchronize()
    o_on = {k: o_on[k].clone() for k in keys}
    eng.set_option("pair_launches", 0)
    off = _trace(eng, banked, T)
    o_off = eng.forward(banked, T=T)
    torch.cuda.synchronize()
    eng.set_option("pair_launches", 1)
    print(name, rows, "pair_launches 1:", on, "0:", off)
    if name == CFG2:
        assert on == ["bank_prep", "obj_qkv", "obj_attn", "obj_tail", "mul_pv", "mul_attn", "mul_tail", "pred_head"]
    if structured:
        assert off[:3] == three and "bank_prep" not in off
    else:
        assert off[:2] == three[1:] and "mul_pl" not in off and "bank_prep" not in off
    assert on == (["bank_prep"] + off[3:] if fused else off)
    for k in keys:
        assert torch.equal(o_on[k], o_off[k]), (name, k)
    assert torch.isfinite(o_on["mdl_outs"]).all()
    # a graph slot replays the fused launch
    slot = eng.make_slot(banked, T=T, graph=True)
    sout = slot.launch()
    torch.cuda.synchronize()
    slot.check()
    for k in keys:
        assert torch.equal(sout[k], o_on[k]), (name, "slot", k)
    # raw features: today's member trace
    grp = eng.make_group([dev], graph=False)
    member = eng.describe_steps(grp.slots[0].batch, grp.slots[0].ws)
    assert _trace(eng, vec, T) == member and "bank_prep" not in member


# ---- 4: the bank loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep"])
def test_lang_bank_loader_and_fed_pipeline(name):
    """`LangBank.loader` batches equal `QueryBank.loader` batches on the shared keys (and carry ARG_KEYS in place of the
    word-level keys); `FedPipeline(..., queries=lang_bank)` over 6 index batches equals the eager vector-form forward of the
    loader's batch bit for bit; a bad index gives zero rows and `check()` raises."""
    eng, cfg, sd, batch, c, dev = build_engine(name)
    B, ncmp = batch["num_cmp_msk"].shape
    T = int(batch["srl_arg_word_mask_len"].max())
    Q, nv = 9, 7
    rows = _query_rows(batch, Q)
    rows["sent_idx"] = torch.arange(Q, dtype=torch.int64)
    pq = synth.make_items(Q, ncmp, 1, prop_dim=4, seg_dim=4, n_gt=8, seed=60)
    rows.update({k: torch.from_numpy(np.ascontiguousarray(pq[k])) for k in dls.PER_QUERY_KEYS})
    qb = dls.QueryBank.from_batches([rows], host_keys=["sent_idx"])
    lbk = dls.LangBank.encode(qb, eng, B, T)
    raw = dls.FeatureBank(cfg, comm_for(c), nv, dtype="f32", n_gt=8)
    raw.put(0, _pool(nv, cfg, c, 17))
    rng = np.random.default_rng(5)
    index = [{"qry_index": torch.from_numpy(rng.integers(0, Q, size=B).astype(np.int32)),
              "vid_index": torch.from_numpy(rng.integers(0, nv, size=(B, ncmp)).astype(np.int32))} for _ in range(6)]
    a_batches, b_batches = list(lbk.loader(index, raw)), list(qb.loader(index, raw))
    torch.cuda.synchronize()
    keys = OUT_KEYS + (SEP_KEYS if eng.sep else ())
    for a, b in zip(a_batches, b_batches):
        assert set(a) == (set(b) - set(WORDS)) | set(ARG[:2 if eng.sep else 1])
        for k in set(a) & set(b):
            assert torch.equal(a[k], b[k]), k
        assert engine_mod.language_kind(a) == "vec"
    eager = []
    for a in a_batches:
        o = eng.forward(a, T=T)
        eager.append({k: o[k].clone() for k in keys})
    torch.cuda.synchronize()
    ex = {k: v for k, v in a_batches[0].items() if k in engine_mod.NSRL_KEYS_I64 + engine_mod.F32_KEYS + ARG + ("verb_ind_in_srl", "new_srl_idxs")}
    spec = {"qry_index": torch.zeros(B, dtype=torch.int32), "vid_index": torch.zeros(B, ncmp, dtype=torch.int32)}
    pipe = engine_mod.FedPipeline(eng, ex, spec, assembler=raw, streams=2, slots_per_stream=1, T=T, queries=lbk)
    assert all(sl.vec and sl.queries is lbk for sl in pipe.slots)
    with pytest.raises(ValueError, match="LangBank"):
        eng.make_slot(ex, T=T, graph=True).feed_from(dls.PackedStaging(spec, n_dev=1), raw, via="device", queries=qb)
    for i, ib in enumerate(index):
        st = pipe.next_staging()
        st.host["qry_index"].copy_(ib["qry_index"])
        st.host["vid_index"].copy_(ib["vid_index"])
        sl = pipe.submit()
        pipe.done(sl).synchronize()
        sl.check()
        for k in keys:
            assert torch.equal(sl.out[k], eager[i][k]), (name, i, k)
    # a bad index: zero rows plus the sticky word
    bad = torch.tensor([0, Q] + [1] * (B - 2), dtype=torch.int32).cuda()[:B]
    got = lbk(bad)
    torch.cuda.synchronize()
    assert not bool(got[ARG[0]][1].any()) and bool(got[ARG[0]][0].any())
    with pytest.raises(L.VogError, match="outside"):
        lbk.check()
    lbk.check()


# ---- 5: staleness -----------------------------------------------------------------------------------------------------------
def test_lang_bank_goes_stale_with_the_weights():
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_sep")
    T = int(batch["srl_arg_word_mask_len"].max())
    qb = dls.QueryBank.from_batches([_query_rows(batch, 5)], host_keys=[])
    lbk = dls.LangBank.encode(qb, eng, 2, T)
    old = {k: lbk.tab[k].clone() for k in ARG}
    lbk.check()
    sd2 = {k: (v * np.float32(1.1) if k.startswith("lstm_encoder.lstm.weight_hh") else v) for k, v in sd.items()}
    eng.load_state_dict(sd2)
    assert lbk.stale() and not lbk.lossless_for(eng)
    with pytest.raises(L.VogError, match="refresh"):
        lbk.check()
    ptrs = {k: lbk.tab[k].data_ptr() for k in ARG}
    lbk.refresh()
    lbk.check()
    fresh = dls.LangBank.encode(qb, eng, 2, T)
    for k in ARG:
        assert lbk.tab[k].data_ptr() == ptrs[k]                        # in place: captured graphs keep their addresses
        assert torch.equal(lbk.tab[k], fresh.tab[k]) and not torch.equal(lbk.tab[k], old[k]), k
    kept_none = dls.LangBank.encode(qb, eng, 2, T, keep_source=False)
    eng.load_state_dict(sd)
    with pytest.raises(L.VogError, match="kept none"):
        kept_none.refresh()
    kept_none.refresh(qb)
    assert torch.equal(kept_none.tab[ARG[0]], old[ARG[0]])


# ---- 6: the evaluator and the CLI -------------------------------------------------------------------------------------------
def _records(blob):
    recs = pickle.loads(blob)
    return (np.array([r["pred_scores"] for r in recs]), np.array([r["pred_boxes"] for r in recs]), np.array([r["pred_cmp"] for r in recs]),
            [r["idx_sent"] for r in recs])


def _assert_close_runs(ref, got, what, loss_lambda=1.0):
    """(loss, metrics, pickle) of a lang_bank run against the query_bank run, to the bound of the forward test: the logits move
    by at most 1.5e-3, a mean of BCE terms has slope <= 1 in every logit, so each loss term moves by at most that (the total
    by (1 + lambda) times it); scores 4e-4; boxes are equal, or near-tie flips counted as `_check_against` counts them (at most
    max(2, 0.5 %)); the metrics are equal where no box and no pred_cmp flipped."""
    print(what, "query_bank", ref[0], ref[1], "lang_bank", got[0], got[1])
    assert set(got[0]) == set(ref[0])
    for k in ref[0]:
        assert abs(got[0][k] - ref[0][k]) <= LOGIT_BOUND * (1.0 + abs(loss_lambda)), (what, k)
    sa, ba, ca, ia = _records(ref[2])
    sb, bb, cb, ib = _records(got[2])
    assert ia == ib and sa.shape == sb.shape
    assert np.abs(sa - sb).max() <= SCORE_BOUND, what
    diff = np.any(ba != bb, axis=-1)
    assert int(diff.sum()) <= max(2, int(0.005 * diff.size)), what
    if not diff.any() and np.array_equal(ca, cb):
        assert got[1] == ref[1], what
    else:
        assert all(abs(got[1][k] - ref[1][k]) <= 0.005 + 2.0 / max(1, len(ia)) for k in ref[1]), what


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_svsq"])
def test_evaluator_lang_bank(name, tmp_path, tmp_path_factory):
    """19 batches of 4, the last a query short: val_graph + query_bank + lang_bank gives the loss, the metrics and the pickle of
    the query_bank run to the bound above, and the bytes of a second lang_bank run; the short tail batch took the eager vector
    form; after a weight reload the bank is re-encoded in place and the run follows the new weights."""
    cfg, sd, comm, sel, dl = _eval_set(name, tmp_path_factory)
    mdl, evl, loss_fn = TDM._evaluator(cfg, sd, comm, sel)
    try:
        ref = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "q", device_metrics=True, val_graph=True, query_bank=True, lang_bank=False)
        got = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "l1", device_metrics=True, val_graph=True, query_bank=True, lang_bank=True)
        st = dict(evl.val_graph_stats)
        lbk = evl._val_graph_cache["lbank"][1]
        assert isinstance(lbk, dls.LangBank) and got[3] == "graph" and st["graph_steps"] == 18 and st["steps"] == 19
        assert st["lang_bank_bytes"] == lbk.nbytes > 0 and st["lang_encode_seconds"] > 0
        assert all(sl.vec and sl.queries is lbk for sl in evl._val_graph_cache["pipe"][1].slots)
        _assert_close_runs(ref, got, name, float(cfg.loss.loss_lambda))
        again = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "l2", device_metrics=True, val_graph=True, query_bank=True, lang_bank=True)
        assert again[:3] == got[:3] and evl._val_graph_cache["lbank"][1] is lbk
        # a weight reload (what Learner.validate does after an epoch): re-encoded, same tables
        sd2 = {k: (v * np.float32(1.1) if k.startswith("lstm_encoder.lstm.weight_hh") else v) for k, v in sd.items()}
        mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
        new = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "l3", device_metrics=True, val_graph=True, query_bank=True, lang_bank=True)
        assert evl._val_graph_cache["lbank"][1] is lbk and not lbk.stale(mdl.engine())
        ref2 = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "q3", device_metrics=True, val_graph=True, query_bank=True, lang_bank=False)
        _assert_close_runs(ref2, new, name + " (new weights)", float(cfg.loss.loss_lambda))
        assert new[0] != got[0]
        # needs query_bank and val_graph
        with pytest.raises(ValueError, match="needs cfg.hip.query_bank"):
            _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "bad", val_graph=True, query_bank=False, lang_bank=True)
    finally:
        cfg.hip["query_bank"], cfg.hip["lang_bank"] = False, False


def test_main_dist_query_bank_lang(capsys, tmp_path):
    """`main_dist --only_val --feature_bank=f16 --query_bank=lang` against `--query_bank=True`: loss, metrics and pickle to the
    bound above, byte-equal to a second lang run; `lang_encode_seconds` is printed."""
    main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
    over = {"mdl.name": "vog", "ds.conc_type": "spat", "mdl.obj_tx.use_rel": True, "mdl.mul_tx.use_rel": True, "train.bsv": 4}
    res = {}
    for uid, kind in (("q", "True"), ("l1", "lang"), ("l2", "lang")):
        main_mod.main_dist("v_" + uid, only_val=True, synthetic_batches=3, feature_bank="f16", feature_bank_videos=32, query_bank=kind,
                           **over, **{"misc.tmp_path": str(tmp_path / uid)})
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{\"uid\"")][-1]
        res[uid] = (json.loads(line), open(tmp_path / uid / "predictions" / ("v_" + uid) / "valid_0.pkl", "rb").read())
    assert res["l1"][0]["query_bank"] == "lang" and res["l1"][0]["queries"] == 11 and res["l1"][0]["lang_encode_seconds"] > 0
    assert res["q"][0]["query_bank"] is True and res["q"][0]["lang_encode_seconds"] == 0.0
    as_run = lambda r: (r[0]["val_loss"], r[0]["val_acc"], r[1])
    _assert_close_runs(as_run(res["q"]), as_run(res["l1"]), "main_dist")
    assert as_run(res["l1"]) == as_run(res["l2"])


# ---- 7: the refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    trn = importlib.import_module("vognet-pytorch_amd.train")
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_spat", cached=True)
    T = int(batch["srl_arg_word_mask_len"].max())
    vec = _vec(eng, dev, T)
    with pytest.raises(ValueError, match="not both"):
        eng.forward({**vec, "srl_arg_words_ind": dev["srl_arg_words_ind"]}, T=T)
    with pytest.raises(ValueError, match="sep / svsq head only"):
        eng.forward({**vec, ARG[1]: torch.zeros(2, 1, eng.desc.lang_enc, device="cuda")}, T=T)
    with pytest.raises(ValueError, match="expected"):
        eng.forward({**vec, ARG[0]: vec[ARG[0]][:, :, :-1].contiguous()}, T=T)
    with pytest.raises(ValueError, match="float32 tensor on the device"):
        eng.forward({**vec, ARG[0]: vec[ARG[0]].cpu()}, T=T)
    with pytest.raises(ValueError, match="make_batched takes the word-level keys"):
        eng.make_batched([vec, vec])
    with pytest.raises(ValueError, match="make_group takes the word-level keys"):
        eng.make_group([vec, vec])
    slot = eng.make_slot(vec, T=T, graph=False)
    with pytest.raises(ValueError, match="same form"):
        slot.update_inputs({k: dev[k] for k in WORDS})
    slot.update_inputs({k: vec[k] for k in ARG if k in vec})
    wslot = eng.make_slot(dev, T=T, graph=False)
    with pytest.raises(ValueError, match="same form"):
        wslot.update_inputs({ARG[0]: vec[ARG[0]]})
    # the training path: the language side is being trained
    tr = trn.FP32Trainer(cfg, comm_for(c), {k: torch.from_numpy(v) for k, v in sd.items()}, None, lr=1e-4)
    with pytest.raises(L.VogError, match="trains the language side"):
        tr._forward(vec)
    # sep: the final hidden state is required
    seng, _, _, sbatch, _, sdev = build_engine("small/vog_sep", cached=True)
    sT = int(sbatch["srl_arg_word_mask_len"].max())
    svec = _vec(seng, sdev, sT)
    with pytest.raises(ValueError, match="needs 'lang_final_hidden'"):
        seng.forward({k: v for k, v in svec.items() if k != ARG[1]}, T=sT)
    with pytest.raises(ValueError, match="comes with"):
        engine_mod.language_kind({ARG[1]: 0})
    # the fp32 plan: a forced one, and one the run-time escalation arrived at
    feng, _, _, fbatch, _, fdev = build_engine("small/vog_spat", tx_dtype="f32")
    assert feng.precise is not None
    with pytest.raises(L.VogError, match="fp32 plan"):
        feng.forward(vec, T=T)
    with pytest.raises(L.VogError, match="fp32 plan"):
        feng.encode_queries({k: fdev[k] for k in LANG5}, 2, T)
    aeng, _, asd, abatch, _, adev = build_engine("small/vog_spat")
    avec = _vec(aeng, adev, T)
    aslot = aeng.make_slot(avec, T=T, graph=True)
    qb = dls.QueryBank.from_batches([_query_rows(abatch, 4)], host_keys=[])
    albk = dls.LangBank.encode(qb, aeng, 2, T)
    req, aeng.tx_request = aeng.tx_request, "f32"                       # what check_logit_scale does when it escalates to fp32
    try:
        aeng.load_state_dict(asd)
    finally:
        aeng.tx_request = req
    assert aeng.plan == "f32"
    with pytest.raises(L.VogError, match="fp32 plan"):
        aeng.forward(avec, T=T)
    with pytest.raises(L.VogError):
        aslot.launch()                                                  # (captured before the reload: refuses like any slot)
    with pytest.raises(L.VogError, match="refresh"):
        albk.check()
    with pytest.raises(L.VogError, match="fp32 plan"):
        albk.refresh()
