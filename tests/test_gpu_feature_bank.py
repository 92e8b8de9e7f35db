"""-m gpu: the device-resident feature bank (dat_loader_simple.FeatureBank -> vog_assemble_from_bank, csrc/assemble.hip):
a batch is `index` [B, ncmp] into the bank's tables plus the per-query keys, and what comes out equals
`vog_assemble_batch` / the reference loader on the same videos bit for bit - from fp32 rows, from f16 rows (decoded; lossless
under the 16-bit plans), through a fed slot's graph and through the evaluation / training loops."""
import importlib

import numpy as np
import pytest
import torch

from oracle import make_golden_assemble as mga
from oracle import vog_oracle as vo
from tests.gpu_util import build_engine, comm_for
from tests.gpu_util import video_pool as _video_pool

pytestmark = pytest.mark.gpu

dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
synth = importlib.import_module("vognet-pytorch_amd.synth")
L = importlib.import_module("vognet-pytorch_amd.lib")
engine_mod = importlib.import_module("vognet-pytorch_amd.engine")

SH = mga.SHAPE
B, NCMP, NPPF, V = SH["B"], SH["ncmp"], SH["nppf0"], 20
FEATS = ("pad_region_feature", "seg_feature_for_frms")
LANG_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
             "srl_arg_inds_msk", "num_cmp_msk")
OUT_KEYS = ("mdl_outs", "mdl_outs_eval", "pred_rec")


def _cfg(conc):
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"ds.conc_type": conc})
    return cfg


def _r16(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float16).float().numpy()


_HOST = {}


def _host_tables():
    """The 12 fixture videos at permuted rows of a 20-row table (the other rows hold other videos, so a wrong row shows),
    and the index that maps every (query, video) back to its row. Built once; never written to."""
    if not _HOST:
        it = mga.items()
        fill = synth.make_items(V, 1, NPPF, prop_dim=SH["prop_dim"], seg_dim=SH["seg_dim"], seed=77)
        host = {k: np.ascontiguousarray(fill[k][:, 0]) for k in dls.BANK_KEYS}
        rows = np.random.default_rng(3).permutation(V)[:B * NCMP]
        for k in dls.BANK_KEYS:
            host[k][rows] = it[k].reshape((B * NCMP,) + it[k].shape[2:])
        _HOST.update(host=host, index=rows.reshape(B, NCMP).astype(np.int32),
                     pq={k: it[k] for k in dls.PER_QUERY_KEYS})
    return _HOST["host"], _HOST["index"], _HOST["pq"]


def _bank(conc, dtype):
    host, _, _ = _host_tables()
    bank = dls.FeatureBank(_cfg(conc), {"num_prop_per_frm": NPPF}, V, dtype=dtype, prop_dim=SH["prop_dim"],
                           seg_dim=SH["seg_dim"], n_gt=host["pad_gt_bboxs"].shape[1])
    bank.put(0, {k: v[:7] for k, v in host.items()})                               # host chunk
    bank.put(7, {k: torch.from_numpy(v[7:]).cuda() for k, v in host.items()})      # device chunk
    return bank


def _gathered(index, pq):
    host, _, _ = _host_tables()
    it = {k: host[k][index] for k in dls.BANK_KEYS}
    it.update(pq)
    return it


def _run(bank, index, pq, **kw):
    res = bank(index, {k: torch.from_numpy(v).cuda() for k, v in pq.items()}, **kw)
    torch.cuda.synchronize()
    bank.check()
    return {k: v.cpu().numpy() for k, v in res.items() if k != "_keepalive"}


def _same(got, ref, keys, dtype="f32", tag=""):
    for k in keys:
        want = _r16(ref[k]) if (dtype == "f16" and k in FEATS) else ref[k]
        assert got[k].shape == want.shape, (tag, k, got[k].shape, want.shape)
        assert np.array_equal(got[k], want.astype(got[k].dtype)), (tag, k)


@pytest.mark.parametrize("conc", ["spat", "temp"])
def test_f32_bank_reproduces_the_reference_fixture(conc):
    """Case 1: the fixture's 12 videos at permuted rows of a 20-row bank, gathered back through `index`: all eight keys equal
    the output of the reference loader methods (tests/golden/assemble__*.npz) bit for bit."""
    _, index, pq = _host_tables()
    g = np.load(mga.path(conc))
    _same(vo.assemble_batch(_gathered(index, pq), conc, synth.NFRM0, NPPF), g, mga.KEYS, tag="oracle on the gathered items")
    got = _run(_bank(conc, "f32"), torch.from_numpy(index).cuda(), pq)
    assert set(mga.KEYS) <= set(got)
    _same(got, g, mga.KEYS)


def _repeat_index():
    _, index, _ = _host_tables()
    idx = index.copy()
    idx[0, 1] = idx[0, 0]
    idx[2] = idx[0][::-1]
    return idx


@pytest.mark.parametrize("conc", ["spat", "temp"])
def test_repeated_videos_within_and_across_queries(conc):
    """Case 2: a video twice inside a query and a query made of another one's videos in reverse order."""
    _, _, pq = _host_tables()
    idx = _repeat_index()
    ref = vo.assemble_batch(_gathered(idx, pq), conc, synth.NFRM0, NPPF)
    _same(_run(_bank(conc, "f32"), torch.from_numpy(idx).cuda(), pq), ref, mga.KEYS)


@pytest.mark.parametrize("conc", ["spat", "temp"])
def test_f16_bank_decodes_to_the_f16_rounded_features(conc):
    """Case 3: features == x.to(float16).float() bit for bit, every other key as from the f32 bank."""
    _, index, pq = _host_tables()
    g = np.load(mga.path(conc))
    bank = _bank(conc, "f16")
    assert bank.tab["pad_region_feature"].dtype == torch.float16 and bank.nbytes < _bank(conc, "f32").nbytes
    got = _run(bank, torch.from_numpy(index).cuda(), pq)
    assert not np.array_equal(got["pad_region_feature"], g["pad_region_feature"])      # (the rounding is visible in fp32)
    _same(got, g, mga.KEYS, dtype="f16")
    _same(_run(bank, torch.from_numpy(_repeat_index()).cuda(), pq),
          vo.assemble_batch(_gathered(_repeat_index(), pq), conc, synth.NFRM0, NPPF), mga.KEYS, dtype="f16")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_sep_is_the_plain_gather(dtype):
    """Case 4: VOG_CONC_SEP - every key is bank_host[k][index], [B, ncmp, ...]: no shift, no re-order."""
    host, _, _ = _host_tables()
    idx = _repeat_index()
    got = _run(_bank("sep", dtype), torch.from_numpy(idx).cuda(), {})
    assert set(dls.BANK_KEYS) <= set(got) and "pad_frm_mask" not in got and "srl_boxes" not in got
    _same(got, {k: host[k][idx] for k in dls.BANK_KEYS}, dls.BANK_KEYS, dtype=dtype)
    fwd = _run(_bank("sep", dtype), torch.from_numpy(idx).cuda(), {}, with_loss_keys=False)
    assert set(fwd) == set(dls.FWD_KEYS)
    _same(fwd, {k: host[k][idx] for k in dls.FWD_KEYS}, dls.FWD_KEYS, dtype=dtype)


@pytest.mark.parametrize("conc", ["spat", "sep"])
def test_index_in_pinned_host_memory_is_read_in_place(conc):
    """Case 5: zero copy - the kernels read a pinned int32 index over the host link; same result as from device memory."""
    _, _, pq = _host_tables()
    idx = _repeat_index()
    bank = _bank(conc, "f16")
    pinned = torch.from_numpy(idx).pin_memory()
    a, _ = bank.args(pinned, {k: torch.from_numpy(v).cuda() for k, v in pq.items()})
    assert a.index == pinned.data_ptr()                       # no staging copy
    got = _run(bank, pinned, pq)
    ref = _run(bank, torch.from_numpy(idx).cuda(), pq)
    assert set(got) == set(ref)
    _same(got, ref, sorted(ref))


@pytest.mark.parametrize("conc,dtype", [("spat", "f32"), ("temp", "f16"), ("sep", "f16")])
def test_an_index_outside_the_bank_is_guarded(conc, dtype):
    """Case 6: index V and -1 form no address - the rows of those videos are zeros (a video without boxes), every other row
    is what it is without them, the sticky word is set and check() raises once; on the host the same index is refused
    before anything is launched."""
    host, index, pq = _host_tables()
    idx = index.copy()
    idx[0, 1], idx[2, 3] = V, -1
    bad = np.zeros((B, NCMP), bool)
    bad[0, 1] = bad[2, 3] = True
    bank = _bank(conc, dtype)
    with pytest.raises(ValueError):
        bank(torch.from_numpy(idx), {k: torch.from_numpy(v).cuda() for k, v in pq.items()})
    with pytest.raises(ValueError):
        bank(torch.from_numpy(idx).pin_memory(), {k: torch.from_numpy(v).cuda() for k, v in pq.items()})
    assert int(bank._bad[0]) == 0
    res = bank(torch.from_numpy(idx).cuda(), {k: torch.from_numpy(v).cuda() for k, v in pq.items()})
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items() if k != "_keepalive"}
    assert int(bank._bad[0]) == 1
    with pytest.raises(L.VogError):
        bank.check()
    bank.check()                                               # reported once
    # expectation: the bad videos as all-zero items without boxes
    it = {k: host[k][np.where(bad, 0, idx)].copy() for k in dls.BANK_KEYS}
    for k in dls.BANK_KEYS:
        it[k][bad] = 0
    if conc == "sep":
        _same(got, it, dls.BANK_KEYS, dtype=dtype)
        return
    it.update(pq)
    ref = vo.assemble_batch(it, conc, synth.NFRM0, NPPF)
    # which video a destination row belongs to: assemble a tag
    tag = dict(it)
    tag["pad_region_feature"] = np.broadcast_to(np.arange(NCMP, dtype=np.float32)[None, :, None, None], it["pad_region_feature"].shape).copy()
    tag["seg_feature_for_frms"] = np.broadcast_to(np.arange(NCMP, dtype=np.float32)[None, :, None, None], it["seg_feature_for_frms"].shape).copy()
    tg = vo.assemble_batch(tag, conc, synth.NFRM0, NPPF)
    row_vid = tg["pad_region_feature"][:, :, 0].astype(int)                  # [B, ncmp * NPv]
    row_bad = np.take_along_axis(bad, row_vid, axis=1)
    seg_bad = np.take_along_axis(bad, tg["seg_feature_for_frms"][:, :, 0].astype(int), axis=1)
    assert row_bad.sum() == 2 * synth.NFRM0 * NPPF and seg_bad.sum() == 2 * synth.NFRM0
    ref["pad_proposals"][row_bad] = 0                          # (no shift is applied to a row that was never read)
    for b in range(B):                                         # their frame-mask rows compare frame 0 against the gt frames
        nb = int(ref["num_box"][b])
        ref["pad_frm_mask"][b][row_bad[b], :nb] = (np.float32(0) != ref["pad_gt_bboxs"][b, None, :nb, 4]).astype(np.uint8)
    for k in ("pad_proposals", "pad_region_feature", "pad_pnt_mask"):
        assert not got[k][row_bad].any(), k
    assert not got["seg_feature_for_frms"][seg_bad].any()
    _same(got, ref, mga.KEYS, dtype=dtype)


def _forward_inputs(name, tx_dtype):
    eng, cfg, sd, batch, c, dev = build_engine(name, tx_dtype=tx_dtype, cached=True)
    Bq, ncmp = batch["num_cmp_msk"].shape
    pd, sdim = int(cfg.mdl.prop_feat_dim), int(cfg.mdl.seg_feat_dim)
    return eng, cfg, batch, c, Bq, ncmp, pd, sdim


def _eager(eng, batch, fwd, T=None):
    full = dict(batch)
    full.update(fwd)
    out = eng.forward({k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in full.items()}, T=T)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in OUT_KEYS}


@pytest.mark.parametrize("name,tx_dtype", [("small/vog_spat", "f16"), ("full/cfg2_vog_spat_gt5_bs4", "f16"),
                                           ("small/vog_spat", "bf16")])
def test_f16_bank_is_lossless_under_the_16_bit_plans(name, tx_dtype):
    """Case 7: the forward on a batch gathered from an f16 bank == the forward on the directly assembled fp32 batch of
    f16-rounded features == the forward on the UNROUNDED fp32 batch, bit for bit (the encoders round every feature to f16
    with one RNE cast before any use; small: cast + GEMM encoders, cfg 2: the fused encoder)."""
    eng, cfg, batch, c, Bq, ncmp, pd, sdim = _forward_inputs(name, tx_dtype)
    assert eng.plan == tx_dtype
    nv = 16
    pool = _video_pool(nv, cfg, c, seed=11, n_gt=100)
    bank = dls.FeatureBank(cfg, comm_for(c), nv, dtype="f16")
    assert bank.lossless_for(eng) and (bank.prop_dim, bank.seg_dim) == (pd, sdim)
    bank.put(0, pool)
    idx = np.random.default_rng(5).integers(0, nv, size=(Bq, ncmp)).astype(np.int32)
    got = bank(torch.from_numpy(idx).cuda(), with_loss_keys=False)
    torch.cuda.synchronize()
    fwd_bank = {k: got[k].cpu().numpy() for k in dls.FWD_KEYS}
    items = {k: pool[k][idx] for k in dls.BANK_KEYS}
    items.update({"target_cmp": np.zeros(Bq, np.int64), "srl_boxes": np.zeros((Bq, 1, 5, 4), np.int64),
                  "srl_boxes_lens": np.zeros((Bq, 1, 5, 4), np.int64)})
    asm = vo.assemble_batch(items, cfg.ds.conc_type, synth.NFRM0, c["nppf0"])
    fwd_f32 = {k: asm[k] for k in dls.FWD_KEYS}
    fwd_r16 = {k: (_r16(asm[k]) if k in FEATS else asm[k]) for k in dls.FWD_KEYS}
    for k in dls.FWD_KEYS:
        assert np.array_equal(fwd_bank[k], fwd_r16[k]), k
    assert not np.array_equal(fwd_r16["pad_region_feature"], fwd_f32["pad_region_feature"])
    o_bank, o_r16, o_f32 = (_eager(eng, batch, f) for f in (fwd_bank, fwd_r16, fwd_f32))
    for k in OUT_KEYS:
        assert torch.equal(o_bank[k], o_r16[k]), ("bank vs rounded", k)
        assert torch.equal(o_bank[k], o_f32[k]), ("bank vs unrounded", k)
    assert torch.isfinite(o_bank["mdl_outs"]).all()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_fed_slot_gathers_from_the_bank_inside_its_graph(dtype):
    """Case 8: `Slot.feed_from(staging, assembler=bank, via="device")` (vog_graph_capture_fed_bank) at the cfg-2 shape: the
    staging buffer holds the video indices and the word-level arrays - under 64 KB - and every launch equals the eager
    forward on the oracle-assembled batch of the same videos bit for bit."""
    name = "full/cfg2_vog_spat_gt5_bs4"
    eng, cfg, batch, c, Bq, ncmp, pd, sdim = _forward_inputs(name, None)
    nv = 64
    pool = _video_pool(nv, cfg, c, seed=13, n_gt=100)
    bank = dls.FeatureBank(cfg, comm_for(c), nv, dtype=dtype)
    assert bank.lossless_for(eng), eng.plan
    bank.put(0, pool)
    dev_a = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    T = int(batch["srl_arg_word_mask_len"].max())
    slot = eng.make_slot(dev_a, T=T, graph=True)
    stg = dls.PackedStaging({"vid_index": np.zeros((Bq, ncmp), np.int32), **{k: np.zeros_like(batch[k]) for k in LANG_KEYS}}, n_dev=1)
    assert stg.nbytes < 64 << 10
    slot.feed_from(stg, assembler=bank, via="device")
    assert set(slot.fed_keys) == set(dls.FWD_KEYS) | set(LANG_KEYS)
    cs = torch.cuda.Stream()
    rng = np.random.default_rng(9)
    outs = []
    for i in range(3):
        idx = rng.integers(0, nv, size=(Bq, ncmp)).astype(np.int32)
        if i == 1:
            idx[0, 1] = idx[0, 0]
        stg.fill({"vid_index": idx})
        stg.fill({k: batch[k] for k in LANG_KEYS})
        stg.upload_on(cs)
        out = slot.launch()
        stg.release()
        slot.consumed().synchronize()
        got = {k: out[k].clone() for k in OUT_KEYS}
        items = {k: pool[k][idx] for k in dls.BANK_KEYS}
        items.update({"target_cmp": np.zeros(Bq, np.int64), "srl_boxes": np.zeros((Bq, 1, 5, 4), np.int64),
                      "srl_boxes_lens": np.zeros((Bq, 1, 5, 4), np.int64)})
        asm = vo.assemble_batch(items, cfg.ds.conc_type, synth.NFRM0, c["nppf0"])
        for k in dls.FWD_KEYS:
            want = _r16(asm[k]) if (dtype == "f16" and k in FEATS) else asm[k]
            assert np.array_equal(slot.inp[k].cpu().numpy(), want), (i, k)
        ref = _eager(eng, batch, {k: asm[k] for k in dls.FWD_KEYS}, T=T)
        for k in OUT_KEYS:
            assert torch.equal(got[k], ref[k]), (i, k)
        outs.append(got)
    slot.check()
    assert not torch.equal(outs[0]["mdl_outs"], outs[1]["mdl_outs"])


def test_evaluation_and_training_loops_run_on_index_batches(tmp_path):
    """Case 9: small model. Six validation batches through `bank.loader` and through a loader of the same batches
    materialised on the host: `Evaluator.forward` returns identical losses and prediction records; two `Learner` training
    steps from either loader end with bit-identical parameters."""
    import pickle
    from oracle import cases
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
    name = "small/vog_spat"
    cfg, sd, batch, c = cases.build(name)
    comm = comm_for(c)
    conc, nppf0 = cfg.ds.conc_type, c["nppf0"]
    Bq, ncmp = batch["num_cmp_msk"].shape
    nv = 24
    pool = _video_pool(nv, cfg, c, seed=17, n_gt=100)
    bank = dls.FeatureBank(cfg, comm, nv, dtype="f32")
    bank.put(0, pool)
    index_batches, host_batches = [], []
    for i in range(6):
        rng = np.random.default_rng(100 + i)
        lang = synth.make_batch(conc, Bq, 1, ncmp=ncmp, vocab_size=c["vocab"], prop_dim=4, seg_dim=4, seed=40 + i, ragged=True)
        small = {k: lang[k] for k in lang if k not in dls.FWD_KEYS}
        pq = synth.make_items(Bq, ncmp, 1, prop_dim=4, seg_dim=4, n_gt=4, seed=60 + i)
        small.update({k: pq[k] for k in dls.PER_QUERY_KEYS})
        small.update({"srl_arg_boxes_mask": small["srl_arg_inds_msk"].copy(),
                      "ann_idx": np.arange(i * Bq, (i + 1) * Bq, dtype=np.int64), "sent_idx": np.arange(i * Bq, (i + 1) * Bq, dtype=np.int64),
                      "permute": np.tile(np.arange(ncmp), (Bq, 1)).astype(np.int64),
                      "permute_inv": np.tile(np.arange(ncmp), (Bq, 1)).astype(np.int64)})
        idx = rng.integers(0, nv, size=(Bq, ncmp)).astype(np.int32)
        index_batches.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**small, "vid_index": idx}.items()})
        items = {k: pool[k][idx] for k in dls.BANK_KEYS}
        items.update({k: pq[k] for k in dls.PER_QUERY_KEYS})
        full = {**small, **vo.assemble_batch(items, conc, synth.NFRM0, nppf0)}
        host_batches.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in full.items()})
    first = next(iter(bank.loader(index_batches[:1])))
    assert all(v.is_cuda for v in first.values()) and set(first) == set(host_batches[0])

    def build():
        sel = sel_mod.get_mdl_loss_eval(cfg)
        mdl = sel["mdl"](cfg=cfg, comm=comm)
        mdl.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in sd.items()})
        return mdl, sel["loss"](cfg, comm), sel["eval"](cfg, comm, torch.device("cuda", 0))

    res = {}
    for tag, dl in (("bank", bank.loader(index_batches)), ("host", host_batches)):
        mdl, loss_fn, evl = build()
        vl, _ = evl(mdl, loss_fn, dl, "valid", rank=0, pred_path=tmp_path / tag)
        res[tag] = ({k: float(v) for k, v in vl.items()}, pickle.loads(open(tmp_path / tag / "valid_0.pkl", "rb").read()))
    assert res["bank"][0] == res["host"][0] and len(res["bank"][1]) == 6 * Bq
    assert res["bank"][1] == res["host"][1]
    params = {}
    for tag, dl in (("bank", bank.loader(index_batches[:2])), ("host", host_batches[:2])):
        mdl, loss_fn, evl = build()
        learn = tu.Learner(uid="B_" + tag, data=tu.DataWrap(path=tmp_path, train_dl=dl, valid_dl=dl), mdl=mdl, loss_fn=loss_fn,
                           cfg=cfg, eval_fn=evl, comm=comm)
        learn.train_epoch()
        assert learn.trainer.num_it == 2
        params[tag] = {k: v.clone() for k, v in learn.trainer.state_dict().items()}
    for k, v in params["host"].items():
        assert torch.equal(v, params["bank"][k]), k
    assert any(k in sd and not torch.equal(v.cpu(), torch.from_numpy(sd[k])) for k, v in params["host"].items())
    bank.check()
