"""-m gpu: `cfg.hip.val_graph` - a validation step as one transfer and one graph launch.

Bottom up: the log kernel alone (`vog_val_log`, csrc/val.hip) and its step guard; the SEP frame mask of the bank gather
against the reference-made fixture; one fed slot whose graph ends in loss + metrics + log (`vog_graph_capture_val`) against the
eager calls; `Evaluator.forward` with `val_graph` against the existing loop - loss, metrics and pickle bytes EQUAL - from host
loaders and bank loaders, at several pipeline geometries, with ragged sentences, after a weight reload, on the fp32 plan (which
keeps the existing loop) and on two ranks. Every comparison is against the existing path or the fixture."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_device_metrics as T
from tests.gpu_util import build_engine
from tests.test_val_graph_host import GOLD, sep_frm_mask

pytestmark = pytest.mark.gpu

L = importlib.import_module("vognet-pytorch_amd.lib")
dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
engine_mod = importlib.import_module("vognet-pytorch_amd.engine")
synth = importlib.import_module("vognet-pytorch_amd.synth")
mdl_conc = importlib.import_module("vognet-pytorch_amd.mdl_conc")

ROWS = 5
SENT_F, SENT_I = -77.0, -77


# ---- 1 / 2: the log kernel alone ------------------------------------------------------------------------------------------
def _log(B, rw):
    log = engine_mod.ValLog("cuda", ROWS, B, loss=True, words=True, rec_words=rw)
    log.loss.fill_(SENT_F)
    log.words.fill_(SENT_I)
    if log.rec is not None:
        log.rec.fill_(SENT_F)
    return log


def _sources(B, rw, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(8, generator=g).cuda(), torch.randint(0, 2 ** 20, (B,), generator=g, dtype=torch.int32).cuda(),
            torch.randn(B, rw, generator=g).cuda() if rw else None)


def _real_rw():
    eng, cfg, sd, batch, c, dev = build_engine("small/vog_spat", cached=True)
    return eng.record_words(batch["num_cmp_msk"].shape[1])


@pytest.mark.parametrize("rw", [0, 5, "real"])
@pytest.mark.parametrize("B", [1, 3, 4, 67])
def test_val_log_writes_only_its_row(B, rw):
    """rows = 5, steps 3, 0, 4 on a non-default stream: written rows are byte-equal to their sources (record widths that
    are no multiple of four words put rows at every 16-byte phase), the others keep the sentinel, markers follow."""
    rw = _real_rw() if rw == "real" else rw
    log = _log(B, rw)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    srcs = {}
    for step in (3, 0, 4):
        srcs[step] = _sources(B, rw, 100 + step)
        st.wait_stream(torch.cuda.current_stream())
        log.write(step, *srcs[step], stream=st)
    st.synchronize()
    log.check()
    assert log.written.cpu().tolist() == [1, 0, 0, 1, 1]
    for r in range(ROWS):
        if r in srcs:
            lo, wo, ro = srcs[r]
            assert torch.equal(log.loss[r].view(torch.int32), lo[:6].view(torch.int32))
            assert torch.equal(log.words[r], wo)
            if rw:
                assert torch.equal(log.rec[r].view(torch.int32), ro.reshape(-1).view(torch.int32))
        else:
            assert bool((log.loss[r] == SENT_F).all()) and bool((log.words[r] == SENT_I).all())
            assert not rw or bool((log.rec[r] == SENT_F).all())
    with pytest.raises(L.VogError, match="never written"):
        log.check_written(ROWS)


@pytest.mark.parametrize("phase", [1, 2, 3])
def test_val_log_sources_and_rows_at_the_same_odd_phase(phase):
    """A source and its row that share a NON-zero 16-byte phase take the head / 16-byte body / tail path: B = 3 with 5-word
    records puts row s of the record log at phase 15 s mod 4 words and row s of the word log at 3 s mod 4; the sources start
    `phase` words into their buffers. Steps chosen so that both logs meet their source's phase (and, in the other rows, miss it)."""
    B, rw = 3, 5
    log = _log(B, rw)
    lo, _, _ = _sources(B, rw, 1)
    g = torch.Generator().manual_seed(50 + phase)
    wbuf = torch.randint(0, 2 ** 20, (8,), generator=g, dtype=torch.int32).cuda()
    rbuf = torch.randn(24, generator=g).cuda()
    wsrc, rsrc = wbuf[phase:phase + B], rbuf[phase:phase + B * rw].view(B, rw)
    assert wsrc.data_ptr() % 16 == 4 * phase and rsrc.data_ptr() % 16 == 4 * phase
    steps = [s for s in range(ROWS) if (15 * s) % 4 == phase or (3 * s) % 4 == phase]
    assert any((15 * s) % 4 == phase for s in steps) and any((3 * s) % 4 == phase for s in steps)
    for s in steps:
        assert (log.rec[s].data_ptr() % 16 == 4 * phase) == ((15 * s) % 4 == phase)
        log.write(s, lo, wsrc, rsrc)
    torch.cuda.synchronize()
    log.check()
    for r in range(ROWS):
        if r in steps:
            assert torch.equal(log.words[r], wsrc) and torch.equal(log.rec[r].view(torch.int32), rsrc.reshape(-1).view(torch.int32)), r
        else:
            assert bool((log.words[r] == SENT_I).all()) and bool((log.rec[r] == SENT_F).all()), r
    assert log.written.cpu().tolist() == [int(r in steps) for r in range(ROWS)]


def test_metrics_launch_writes_its_row_of_the_logs():
    """vog_gmetric_args.log: the metrics launch writes the step's row itself (what a fed graph captures) - the word row
    equals the plain launch's words, loss and record rows equal their sources, the slot's own result words are written too;
    a step outside the log writes no row and sets the sticky word."""
    import ctypes as C
    from tests import metrics_util as U
    conc = "spat"
    ev = U.CLS[conc](U.cfg_for(), {"num_prop_per_frm": 5})
    arr = {k: v[:63] for k, v in U.fixture_arrays(conc).items()}          # (63: the last workgroup is one record short)
    want, (rec, cols, _) = T.run_kernel(ev, arr, conc)
    B, rw = rec.shape
    assert bool((want != 0).any())
    lo, _, _ = _sources(B, 0, 3)
    tab, _ = ev.device_table("cuda")
    st = torch.cuda.Stream()
    for step, ok in ((3, True), (ROWS, False), (-1, False), (0, True)):
        log = _log(B, rw)
        res = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        stp = torch.tensor([step], dtype=torch.int32, device="cuda")
        a = L.GMetricArgs()
        a.rec = L.ptr(rec)
        a.idx_sent, a.idx_verbs, a.cmp_msk, a.targ_cmp = (L.ptr(c) for c in cols)
        a.tab, a.result = C.pointer(tab), L.ptr(res)
        a.B, a.ncmp, a.nsrl, a.nfrm0 = B, arr["cmp_msk"].shape[1], arr["pred_scores"].shape[1], arr["pred_scores"].shape[3]
        a.conc_type, a.prob_thresh = L.CONC_TYPE[conc], float(ev.prob_thresh)
        la = log.args(stp, lo, res, rec)                  # (word_src is not read by this form: the waves write the row)
        a.log = C.addressof(la)
        torch.cuda.synchronize()
        L.check(L.load().vog_ground_metrics(C.byref(a), L.stream_ptr(st)), "vog_ground_metrics")
        st.synchronize()
        assert np.array_equal(res.cpu().numpy(), want), step
        if ok:
            log.check()
            assert log.written.cpu().tolist() == [int(r == step) for r in range(ROWS)]
            assert np.array_equal(log.words[step].cpu().numpy(), want)
            assert torch.equal(log.loss[step].view(torch.int32), lo[:6].view(torch.int32))
            assert torch.equal(log.rec[step].view(torch.int32), rec.reshape(-1).view(torch.int32))
            others = [r for r in range(ROWS) if r != step]
            assert bool((log.words[others] == SENT_I).all()) and bool((log.rec[others] == SENT_F).all()) and bool((log.loss[others] == SENT_F).all())
        else:
            assert bool((log.words == SENT_I).all()) and bool((log.rec == SENT_F).all()) and bool((log.loss == SENT_F).all())
            assert log.written.cpu().tolist() == [0] * ROWS
            with pytest.raises(L.VogError, match="outside"):
                log.check()


def test_val_log_parts_are_optional():
    log = engine_mod.ValLog("cuda", ROWS, 4, loss=True, words=False, rec_words=0)
    lo, wo, _ = _sources(4, 0, 1)
    log.write(2, lo, wo, None)                        # (a source without a log is ignored)
    torch.cuda.synchronize()
    assert log.words is None and log.rec is None and torch.equal(log.loss[2], lo[:6]) and log.written.cpu().tolist() == [0, 0, 1, 0, 0]


@pytest.mark.parametrize("step", [-1, ROWS])
def test_a_step_outside_the_log_is_guarded(step):
    """The guard of an index: no address is formed from it, nothing is written, the sticky word is set and the Python
    surface raises at its next check (once)."""
    rw = 5
    log = _log(4, rw)
    log.write(step, *_sources(4, rw, 7))
    torch.cuda.synchronize()
    assert bool((log.loss == SENT_F).all()) and bool((log.words == SENT_I).all()) and bool((log.rec == SENT_F).all())
    assert log.written.cpu().tolist() == [0] * ROWS and int(log._bad[0]) == 1
    with pytest.raises(L.VogError, match="outside"):
        log.check()
    log.check()
    log.write(1, *_sources(4, rw, 8))                 # the log stays usable
    torch.cuda.synchronize()
    log.check()
    assert log.written.cpu().tolist() == [0, 1, 0, 0, 0]


# ---- 3: the SEP frame mask of the bank gather -----------------------------------------------------------------------------
def _sep_bank(conc, dtype):
    g = np.load(GOLD)
    V, NPv, G = g["pad_proposals"].shape[0], g["pad_proposals"].shape[1], g["pad_gt_bboxs"].shape[1]
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"ds.conc_type": conc})
    nppf = NPv // synth.NFRM0
    bank = dls.FeatureBank(cfg, {"num_prop_per_frm": nppf}, V, dtype=dtype, prop_dim=8, seg_dim=8, n_gt=G)
    rng = np.random.default_rng(4)
    bank.put(0, {"pad_proposals": g["pad_proposals"], "pad_pnt_mask": g["pad_pnt_mask"], "pad_gt_bboxs": g["pad_gt_bboxs"],
                 "num_box": g["num_box"], "pad_region_feature": rng.standard_normal((V, NPv, 8), dtype=np.float32),
                 "seg_feature_for_frms": rng.standard_normal((V, synth.NFRM0, 8), dtype=np.float32)})
    return cfg, bank, g, nppf


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("conc", ["sep", "svsq"])
def test_sep_frame_mask_from_the_bank_equals_the_reference_fixture(conc, dtype):
    cfg, bank, g, nppf = _sep_bank(conc, dtype)
    V = g["num_box"].shape[0]
    index = np.arange(V, dtype=np.int32).reshape(V, 1) if conc == "svsq" else np.array([[0, 1, 2, 3], [4, 5, 1, 1], [3, 2, 0, 4]], np.int32)
    res = bank(torch.from_numpy(index).cuda(), {}, with_loss_keys=True, sep_frm_mask=True)
    torch.cuda.synchronize()
    bank.check()
    got = res["pad_frm_mask"].cpu().numpy()
    assert got.shape == index.shape + g["pad_frm_mask"].shape[1:]
    assert np.array_equal(got, g["pad_frm_mask"][index])
    assert (got == 0).any()
    # the plain gather is unchanged without the switch
    assert "pad_frm_mask" not in bank(torch.from_numpy(index).cuda(), {}, with_loss_keys=True)
    # LossB_SEP on the bank batch == on the host-materialised batch, bit for bit
    B, ncmp = index.shape
    nsrl, NPv = 5, g["pad_proposals"].shape[1]
    rng = np.random.default_rng(11)
    small = {"srl_boxes": rng.integers(0, g["pad_gt_bboxs"].shape[1], size=(B, 1, nsrl, 4)).astype(np.int64),
             "srl_boxes_lens": (rng.uniform(size=(B, 1, nsrl, 4)) < 0.7).astype(np.int64),
             "srl_arg_boxes_mask": (rng.uniform(size=(B, 1, nsrl)) < 0.8).astype(np.int64),
             "target_cmp": rng.integers(0, ncmp, size=(B,)).astype(np.int64), "num_cmp_msk": np.ones((B, ncmp), np.int64),
             "verb_cmp": (rng.uniform(size=(B, ncmp)) < 0.5).astype(np.int64),
             "verb_cross_cmp_msk": np.ones((B, ncmp, ncmp), np.int64)}
    out = {"mdl_outs": torch.from_numpy(rng.standard_normal((B, ncmp, nsrl, NPv), dtype=np.float32)).cuda(),
           "vidf_outs": torch.from_numpy(rng.standard_normal((B, ncmp), dtype=np.float32)).cuda()}
    loss_fn = mdl_conc.LossB_SEP(cfg, {"num_prop_per_frm": nppf})
    host = {"pad_proposals": g["pad_proposals"][index], "pad_gt_bboxs": g["pad_gt_bboxs"][index],
            "pad_pnt_mask": g["pad_pnt_mask"][index], "pad_frm_mask": np.stack([[sep_frm_mask(g["pad_proposals"][v], g["pad_pnt_mask"][v], g["pad_gt_bboxs"][v], int(g["num_box"][v])) for v in row] for row in index])}
    dev_small = {k: torch.from_numpy(v).cuda() for k, v in small.items()}
    a = loss_fn(out, {**dev_small, **{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}})
    a = {k: v.clone() for k, v in a.items()}
    b = loss_fn(out, {**dev_small, **{k: v for k, v in res.items() if k != "_keepalive"}})
    torch.cuda.synchronize()
    for k in ("loss", "mdl_out_loss", "verb_loss"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert float(a["mdl_out_loss"]) > 0


# ---- shared evaluation sets -------------------------------------------------------------------------------------------------
_SETS = {}


def _eval_set(name, tmp_path_factory, n_batches=19):
    """(cfg, sd, comm, sel, dl) of make_eval_set, built once per case (19 batches of 4, the last a query short); read only."""
    if name not in _SETS:
        _SETS[name] = T.make_eval_set(name, tmp_path_factory.mktemp("ann_" + name.replace("/", "_")), n_batches=n_batches, B=4, distinct=5)
    return _SETS[name]


def _run(cfg, mdl, evl, loss_fn, dl, out_dir, **hip):
    for k, v in {"device_metrics": False, "val_pickle": True, "batch_requests": 1, "val_graph": False, **hip}.items():
        cfg.hip[k] = v
    with torch.no_grad():
        loss, acc = evl(mdl, loss_fn, dl, "valid", rank=0, pred_path=out_dir)
    torch.cuda.synchronize()
    f = os.path.join(str(out_dir), "valid_0.pkl")
    return ({k: float(v) for k, v in loss.items()}, {k: float(v) for k, v in acc.items()},
            open(f, "rb").read() if os.path.isfile(f) else None, evl.val_path)


COMBOS = ({}, {"device_metrics": True}, {"device_metrics": True, "val_pickle": False})


def _assert_same(ref, got, what):
    print(what, "existing", ref[0], ref[1], "val_graph", got[0], got[1])
    assert got[3] == "graph" and ref[3] == "eager", what
    assert got[0] == ref[0] and set(ref[0]) >= {"loss", "mdl_out_loss"}, what
    assert got[1] == ref[1], what
    assert got[2] == ref[2], what


# ---- 4: one slot with an epilogue -----------------------------------------------------------------------------------------------
def test_one_fed_slot_with_an_epilogue(tmp_path_factory):
    """small/vog_spat, three launches with different batches and out-of-order steps: the loss row equals loss_fn(out, batch)
    bitwise, the word row equals Evaluator._ground_metrics, the record row equals the eager records."""
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    eng = mdl.engine()
    first = dl[0]
    B, ncmp = first["num_cmp_msk"].shape
    want = list(dict.fromkeys(list(engine_mod.NSRL_KEYS_I64 + engine_mod.F32_KEYS) + [k for k, _ in engine_mod.Epilogue.LOSS_KEYS] +
                              list(engine_mod.Epilogue.METRIC_KEYS)))
    rw = eng.record_words(ncmp)
    log = engine_mod.ValLog("cuda", ROWS, B, loss=True, words=True, rec_words=rw)
    epi = engine_mod.Epilogue(log, loss_fn=loss_fn, grnd_eval=evl.grnd_eval)
    spec = {k: first[k] for k in want}
    spec["val_step"] = torch.zeros(4, dtype=torch.int32)
    T_max = int(first["srl_arg_word_mask_len"].max())
    slot = eng.make_slot({k: first[k] for k in want}, T=T_max, graph=True)
    stg = dls.PackedStaging(spec, n_dev=1)
    slot.feed_from(stg, via="device", epilogue=epi)
    assert len(want) + 1 <= L.MAX_COPY_SEGS
    cs = torch.cuda.Stream()
    for i, step in enumerate((3, 0, 4)):
        hb = dl[i + 1]
        stg.fill({k: hb[k] for k in want})
        stg.host["val_step"][0] = step
        stg.upload_on(cs)
        slot.launch()
        stg.release()
        slot.consumed().synchronize()
    slot.check()
    log.check()
    assert log.written.cpu().tolist() == [1, 0, 0, 1, 1]
    for i, step in enumerate((3, 0, 4)):
        batch = {k: v.cuda() for k, v in dl[i + 1].items()}
        with torch.no_grad():
            out = mdl(batch, T=T_max)
            ld = loss_fn(out, batch)
            rec = evl._records(out, batch)
            words = evl._ground_metrics(rec, batch, ncmp, int(eng.desc.nsrl), B)
        torch.cuda.synchronize()
        assert torch.equal(log.loss[step, 0].view(torch.int32), ld["loss"].view(torch.int32)), step
        assert torch.equal(log.loss[step, 1].view(torch.int32), ld["mdl_out_loss"].view(torch.int32)), step
        assert torch.equal(log.words[step], words), step
        assert torch.equal(log.rec[step].view(torch.int32), rec.reshape(-1).view(torch.int32)), step
    assert bool((log.words[[3, 0, 4]] != 0).any())
    assert not torch.equal(log.rec[3], log.rec[0])


# ---- 5: Evaluator.forward, host loader --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "small/vog_svsq", "small/vog_sep"])
def test_evaluator_val_graph_equals_the_existing_loop(name, tmp_path, tmp_path_factory):
    cfg, sd, comm, sel, dl = _eval_set(name, tmp_path_factory)
    assert len(dl) == 19 and int(dl[-1]["num_cmp_msk"].shape[0]) == 3
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    for i, hip in enumerate(COMBOS):
        ref = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / f"e{i}", **hip)
        got = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / f"g{i}", val_graph=True, **hip)
        _assert_same(ref, got, (name, hip))
        assert (ref[2] is None) == (hip.get("val_pickle") is False)
        assert 0 < ref[1]["avg1"] < 1
    with pytest.raises(ValueError, match="batch_requests"):
        _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "r", val_graph=True, batch_requests=2)


# ---- 6: Evaluator.forward, bank loader -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("small/vog_spat", "f32"), ("small/vog_svsq", "f16")])
def test_evaluator_val_graph_from_a_bank_loader(name, dtype, tmp_path, tmp_path_factory):
    """`bank.loader(index_batches)` through the existing loop and through val_graph (the staging buffer then carries the video
    indices and the small keys only); repeated videos inside a query and across batches."""
    cfg, sd, comm, sel, dl = _eval_set(name, tmp_path_factory)
    nv = 24
    nppf0 = comm["num_prop_per_frm"]
    it = synth.make_items(nv, 1, nppf0, prop_dim=int(cfg.mdl.prop_feat_dim), seg_dim=int(cfg.mdl.seg_feat_dim), seed=17)
    bank = dls.FeatureBank(cfg, comm, nv, dtype=dtype)
    bank.put(0, {k: np.ascontiguousarray(it[k][:, 0]) for k in dls.BANK_KEYS})
    drop = set(dls.BANK_KEYS) | {"pad_frm_mask"}
    index_batches = []
    for i, hb in enumerate(dl):
        b, ncmp = hb["num_cmp_msk"].shape
        idx = np.random.default_rng(300 + i).integers(0, nv, size=(b, ncmp)).astype(np.int32)
        if ncmp > 1:
            idx[0, 1] = idx[0, 0]
        if i % 3 == 1:
            idx[:] = index_batches[-1]["vid_index"].numpy()[:b]
        index_batches.append({**{k: v for k, v in hb.items() if k not in drop}, "vid_index": torch.from_numpy(idx)})
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    for i, hip in enumerate(COMBOS):
        ref = _run(cfg, mdl, evl, loss_fn, bank.loader(index_batches), tmp_path / f"e{i}", **hip)
        got = _run(cfg, mdl, evl, loss_fn, bank.loader(index_batches), tmp_path / f"g{i}", val_graph=True, **hip)
        _assert_same(ref, got, (name, dtype, hip))
        assert (ref[2] is None) == (hip.get("val_pickle") is False) and ref[0]["loss"] > 0


# ---- 7: geometries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(1, 1), (2, 2)])
def test_pipeline_geometries(geometry, tmp_path, tmp_path_factory):
    """Slot reuse and ordering: 19 batches through 1 and through 4 slots."""
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    ref = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "e", device_metrics=True)
    evl.VAL_GRAPH_GEOMETRY = geometry

    class Loader:                                      # neither a list nor a bank loader (a DataLoader's surface)
        def __len__(self):
            return len(dl)

        def __iter__(self):
            return iter(dl)

    got = _run(cfg, mdl, evl, loss_fn, Loader() if geometry == (2, 2) else dl, tmp_path / "g", device_metrics=True, val_graph=True)
    _assert_same(ref, got, geometry)
    pipe = evl._val_graph_cache["pipe"][1]
    assert (pipe.n_streams, pipe.per) == geometry and len(pipe.slots) == geometry[0] * geometry[1]
    assert 0 < ref[1]["avg1"] < 1


# ---- 8: ragged sentences ------------------------------------------------------------------------------------------------------------
LANG = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture", "srl_arg_inds_msk")


def _ragged(dl, cfg, comm, always_longest):
    """The loader with sentences of 6 .. 18 tokens (arguments 0 and 1 stay real: the annotations ground them). With
    `always_longest` query 0 of every batch has the 18 tokens of the longest sentence."""
    out = []
    for i, hb in enumerate(dl):
        b, ncmp = hb["num_cmp_msk"].shape
        rng = np.random.default_rng(700 + i)
        lens = [synth.ragged_arg_lens(rng, 6, 17 if always_longest or i else 18) for _ in range(4)]
        if always_longest or i == 0:
            lens[0 if always_longest else 2] = [5, 4, 5, 4, 0]
        lang = synth.make_batch(cfg.ds.conc_type, 4, comm["num_prop_per_frm"], ncmp=ncmp, vocab_size=comm["vocab_size"], prop_dim=4,
                                seg_dim=4, seed=800 + i, arg_lens=lens)
        nb = dict(hb)
        for k in LANG:
            nb[k] = torch.from_numpy(np.ascontiguousarray(lang[k][:b]))
        nb["srl_arg_boxes_mask"] = hb["srl_arg_boxes_mask"] * nb["srl_arg_inds_msk"]
        out.append(nb)
    return out


def test_ragged_sentences(tmp_path, tmp_path_factory):
    """Every batch holding a sentence of T_max: equality. A batch whose own longest sentence is shorter runs at its own T
    in the existing loop and at T_max in the graph (other GEMM tile choices): equal metrics, losses within the forward's
    parity bound of 1e-3."""
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    same_T = _ragged(dl, cfg, comm, True)
    assert all(int(b["srl_arg_word_mask_len"].max()) == 18 for b in same_T) and len({int(b["srl_arg_word_mask_len"].min()) for b in same_T}) > 1
    ref = _run(cfg, mdl, evl, loss_fn, same_T, tmp_path / "e", device_metrics=True)
    got = _run(cfg, mdl, evl, loss_fn, same_T, tmp_path / "g", device_metrics=True, val_graph=True)
    _assert_same(ref, got, "every batch at T_max")
    own_T = _ragged(dl, cfg, comm, False)
    assert len({int(b["srl_arg_word_mask_len"].max()) for b in own_T}) > 2
    ref = _run(cfg, mdl, evl, loss_fn, own_T, tmp_path / "e2", device_metrics=True)
    got = _run(cfg, mdl, evl, loss_fn, own_T, tmp_path / "g2", device_metrics=True, val_graph=True)
    print("own T: existing", ref[0], ref[1], "val_graph", got[0], got[1])
    assert got[3] == "graph" and got[1] == ref[1]
    for k, v in ref[0].items():
        assert abs(got[0][k] - v) <= 1e-3 * abs(v), (k, got[0][k], v)


# ---- 9: weights re-finalised between two validations ----------------------------------------------------------------------------------
def test_weights_reloaded_between_two_validations(tmp_path, tmp_path_factory):
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    first = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "g1", device_metrics=True, val_graph=True)
    old_pipe = evl._val_graph_cache["pipe"][1]
    again = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "g1b", device_metrics=True, val_graph=True)
    assert evl._val_graph_cache["pipe"][1] is old_pipe and again[:3] == first[:3]           # reused while the weights stay
    sd2 = {k: (v * np.float32(1.25) if k.startswith("lin2.") else v) for k, v in sd.items()}
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
    got = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "g2", device_metrics=True, val_graph=True)
    assert evl._val_graph_cache["pipe"][1] is not old_pipe
    ref = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "e2", device_metrics=True)
    _assert_same(ref, got, "new weights")
    assert got[0] != first[0]


# ---- 10: the fp32 plan keeps the existing loop ----------------------------------------------------------------------------------------
def test_fp32_plan_takes_the_existing_loop(tmp_path, tmp_path_factory):
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    import copy
    cfg = copy.deepcopy(cfg)
    cfg.hip.tx_dtype = "f32"
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    assert mdl.engine().precise is not None
    ref = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "e", device_metrics=True)
    got = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "g", device_metrics=True, val_graph=True)
    assert got[3] == "eager" and got[:3] == ref[:3]
    eng = mdl.engine()
    slot = eng.make_slot({k: v for k, v in dl[0].items()}, graph=True)
    with pytest.raises(L.VogError, match="16-bit plan"):
        slot.feed_from(dls.PackedStaging({"val_step": torch.zeros(4, dtype=torch.int32)}, n_dev=1), via="device",
                       epilogue=engine_mod.Epilogue(engine_mod.ValLog("cuda", 2, 4)))


# ---- 11: two ranks on the one GPU -----------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, name, tmp, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    D = importlib.import_module("vognet-pytorch_amd.dist")
    cfg, sd, comm, sel, dl = T.make_eval_set(name, os.path.join(tmp, f"ann{rank}"))
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    idx = list(D.shard_indices(len(dl), rank, world))
    if (len(dl) - 1) in idx:
        idx = [i for i in idx if i != len(dl) - 1] + [len(dl) - 1]
    cfg.hip.device_metrics, cfg.hip.val_pickle, cfg.hip.val_graph = True, True, True
    with torch.no_grad():
        loss, acc = evl(mdl, loss_fn, [dl[i] for i in idx], "valid", rank=rank, pred_path=os.path.join(tmp, "pred"))
    torch.cuda.synchronize()
    if rank == 0:
        q.put(({k: float(v) for k, v in acc.items()}, evl.val_path))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_val_graph_give_the_single_rank_result(tmp_path):
    """World 2 (gloo) on the one GPU: each log is exchanged once, rank-major; rank 0's metrics and pickle equal the single-rank
    existing path's (the wrapped-around duplicate batch of the padded shard loses to its first copy)."""
    import pickle
    import torch.multiprocessing as mp
    name, world = "small/vog_spat", 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = T._free_port()
    ps = [ctx.Process(target=_rank_worker, args=(r, world, port, name, str(tmp_path), q)) for r in range(world)]
    for p in ps:
        p.start()
    got, path = q.get(timeout=300)
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert path == "graph"
    cfg, sd, comm, sel, dl = T.make_eval_set(name, tmp_path / "ann")
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    one = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "one", device_metrics=True)
    assert got == one[1] and 0 < got["avg1"] < 1
    two = pickle.loads((tmp_path / "pred" / "valid_0.pkl").read_bytes())
    ref = pickle.loads(one[2])
    # the padded shard repeats batch 0 on rank 1: the merged pickle is the single-rank one plus that copy, rank-major
    assert len(two) == len(ref) + 4 and two[:12] == ref[:12]
    by_sent = {r["idx_sent"]: r for r in ref}
    assert all(r == by_sent[r["idx_sent"]] for r in two) and {r["idx_sent"] for r in two} == set(by_sent)
