"""-m gpu: the query bank - the per-query part of a batch gathered on the device from `qry_index`.

Bottom up: `vog_gather_rows` alone against `table[idx]` at every access width, between guard bands; its out-of-range guard; one
fed slot whose graph starts with the gather (`vog_graph_capture_desc`) against the eager calls, with the override rule;
`Evaluator.forward` with `val_graph` + `query_bank` against `val_graph` alone and the existing loop - loss, metrics and pickle
bytes EQUAL - from a host loader and from bank loaders; a weight reload between two validations; `QueryBank.loader` against
`BankLoader` and one training step on either batch. The feature is a byte copy in front of unchanged kernels: every comparison
is bitwise."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests import test_gpu_device_metrics as T
from tests.test_gpu_val_graph import COMBOS, _assert_same, _eval_set, _run

pytestmark = pytest.mark.gpu

L = importlib.import_module("vognet-pytorch_amd.lib")
dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
engine_mod = importlib.import_module("vognet-pytorch_amd.engine")
synth = importlib.import_module("vognet-pytorch_amd.synth")

ROW_BYTES = (1, 4, 8, 12, 16, 24, 40, 160, 808, 3200)
GUARD, PATTERN = 64, 0xA5


# ---- 1: the gather alone ----------------------------------------------------------------------------------------------------
def _launch(B, Q, keys, idx, pinned, seed):
    """One vog_gather_rows launch over byte buffers. keys: (row_bytes, table offset, destination offset, per_batch) - the
    offsets are from a 16-byte boundary. Checks every destination against table[idx] (a per-batch key: against its source)
    and the guard bands on both sides of it."""
    g = torch.Generator().manual_seed(seed)
    a = L.GatherArgs()
    index = torch.from_numpy(idx.astype(np.int32))
    index = index.pin_memory() if pinned else index.cuda()
    a.index, a.B, a.Q, a.n_keys = index.data_ptr(), B, Q, len(keys)
    held = []
    for i, (rb, toff, doff, per_batch) in enumerate(keys):
        rows_t, rows_d = (1, 1) if per_batch else (Q, B)
        tbuf = torch.randint(0, 256, (rows_t * rb + 32,), generator=g, dtype=torch.uint8).cuda()
        dbuf = torch.full((GUARD + doff + rows_d * rb + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert tbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
        tab = tbuf[toff:toff + rows_t * rb].view(rows_t, rb)
        dst = dbuf[GUARD + doff:GUARD + doff + rows_d * rb].view(rows_d, rb)
        a.keys[i].table, a.keys[i].dst, a.keys[i].row_bytes, a.keys[i].per_batch = tab.data_ptr(), dst.data_ptr(), rb, int(per_batch)
        held.append((tab, dst, dbuf, doff, rows_d * rb, per_batch))
    torch.cuda.synchronize()
    L.check(L.load().vog_gather_rows(C.byref(a), L.stream_ptr()), "vog_gather_rows")
    torch.cuda.synchronize()
    gi = torch.from_numpy(idx.astype(np.int64)).cuda()
    for i, (tab, dst, dbuf, doff, nb, per_batch) in enumerate(held):
        want = tab if per_batch else tab[gi]
        assert torch.equal(dst, want), (i, keys[i])
        assert bool((dbuf[:GUARD + doff] == PATTERN).all()) and bool((dbuf[GUARD + doff + nb:] == PATTERN).all()), (i, keys[i])


OFFSETS = ((0, 0), (8, 8), (4, 4))
KEYS_32 = [(rb, t, d, False) for (t, d) in OFFSETS for rb in ROW_BYTES] + [(16, 0, 0, True), (20, 0, 0, True)]
KEYS_7 = [(1, 0, 0, False), (12, 8, 4, False), (16, 0, 0, False), (808, 8, 0, False), (3200, 0, 8, False), (16, 0, 0, True), (20, 4, 4, True)]


@pytest.mark.parametrize("Q", [1, 5, 1000])
@pytest.mark.parametrize("B", [1, 3, 4, 67])
def test_gather_rows_equals_table_of_index(B, Q):
    """Row lengths 1 B to 3200 B, 1 / 7 / 32 keys per launch, repeated rows, the index in device and in pinned host memory,
    tables and destinations 0, 8 and 4 bytes off a 16-byte boundary (the 16-, 8-, 4- and 1-byte paths), two per-batch keys."""
    assert len(KEYS_32) == L.MAX_GATHER_KEYS
    rng = np.random.default_rng(31 * B + Q)
    idx = rng.integers(0, Q, size=B)
    if B >= 3:
        idx[1] = idx[0]                                   # a repeated row
        idx[-1] = Q - 1                                   # the last row of the table
    for pinned in (False, True):
        for j, rb in enumerate(ROW_BYTES):                # one key per launch, every row length
            _launch(B, Q, [(rb,) + OFFSETS[j % 3] + (False,)], idx, pinned, seed=j)
        _launch(B, Q, KEYS_7, idx, pinned, seed=50)
        _launch(B, Q, KEYS_32, idx, pinned, seed=60)


# ---- 2: rows outside the bank -----------------------------------------------------------------------------------------------
def test_a_row_outside_the_query_bank_is_guarded():
    """Rows -1 and Q in a batch of 4 form no address: their destination rows are zeros, the two good rows are right, the
    sticky word is set and check() raises once; on the host the same index is refused before anything is launched."""
    Q = 5
    rng = np.random.default_rng(3)
    cols = {"a": rng.integers(1, 2 ** 40, size=(Q, 3)).astype(np.int64), "b": rng.integers(1, 255, size=(Q, 5)).astype(np.uint8),
            "c": rng.integers(1, 2 ** 40, size=(Q,)).astype(np.int64)}
    qb = dls.QueryBank(Q, cols, host_keys=())
    qb.put(0, cols)
    assert qb.nbytes == Q * (24 + 5 + 8) and set(qb.keys) == set(cols)
    bad = np.array([1, -1, Q, 3])
    for t in (torch.from_numpy(bad), torch.from_numpy(bad.astype(np.int32)).pin_memory()):
        with pytest.raises(ValueError, match="outside"):
            qb(t)
    assert int(qb._bad[0]) == 0
    out = {k: torch.full((4,) + v.shape[1:], -1, dtype=torch.from_numpy(v).dtype, device="cuda") for k, v in cols.items()}
    res = qb(torch.from_numpy(bad).cuda(), out=out)
    torch.cuda.synchronize()
    for k, v in cols.items():
        got = res[k].cpu().numpy()
        assert res[k].data_ptr() == out[k].data_ptr()
        assert not got[1].any() and not got[2].any(), k
        assert np.array_equal(got[0], v[1]) and np.array_equal(got[3], v[3]), k
    assert int(qb._bad[0]) == 1
    with pytest.raises(L.VogError, match="outside"):
        qb.check()
    qb.check()                                             # reported once
    good = qb(torch.tensor([4, 0, 0], dtype=torch.int64))  # the bank stays usable; a host int64 index is converted
    torch.cuda.synchronize()
    qb.check()
    assert np.array_equal(good["a"].cpu().numpy(), cols["a"][[4, 0, 0]])


# ---- shared: index batches over a feature bank ----------------------------------------------------------------------------------
def _bank_and_index_batches(cfg, comm, dl, dtype, nv=24):
    """A feature bank of `nv` synthetic videos and the loader's batches with the visual / ground-truth keys replaced by
    `vid_index` (repeated videos inside a query and across batches)."""
    it = synth.make_items(nv, 1, comm["num_prop_per_frm"], prop_dim=int(cfg.mdl.prop_feat_dim), seg_dim=int(cfg.mdl.seg_feat_dim), seed=17)
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
    return bank, index_batches


# ---- 3: one fed slot with an epilogue ---------------------------------------------------------------------------------------
def test_one_query_bank_slot_with_an_epilogue(tmp_path_factory):
    """small/vog_spat from an f32 feature bank; the staging buffer holds {qry_index, val_step} only and `vid_index` is a column
    of the query bank. Three launches with out-of-order steps and rows taken from all over the bank: loss, word and record
    rows equal the eager calls on the same rows bit for bit. A fourth launch from a staging buffer that also carries
    `target_cmp`, with other values than the column's: the staged values win."""
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    eng = mdl.engine()
    bank, index_batches = _bank_and_index_batches(cfg, comm, dl, "f32")
    full = index_batches[:5]
    first = full[0]
    B, ncmp = first["num_cmp_msk"].shape
    produced = set(dls.BANK_KEYS) | {"pad_frm_mask"}
    want = list(dict.fromkeys(list(engine_mod.NSRL_KEYS_I64 + engine_mod.F32_KEYS) + [k for k, _ in engine_mod.Epilogue.LOSS_KEYS] +
                              list(engine_mod.Epilogue.METRIC_KEYS)))
    cols = ["vid_index"] + list(dls.PER_QUERY_KEYS) + [k for k in want if k not in produced and k not in dls.PER_QUERY_KEYS]
    qb = dls.QueryBank.from_batches(full, keys=cols)
    assert qb.Q == 5 * B and "vid_index" in qb.keys and set(qb.host_keys) == set(evl.META_KEYS) & set(cols)
    rows_all = {k: torch.cat([bt[k] for bt in full]) for k in full[0]}
    rw = eng.record_words(ncmp)
    ROWS = 5
    log = engine_mod.ValLog("cuda", ROWS, B, loss=True, words=True, rec_words=rw)
    epi = engine_mod.Epilogue(log, loss_fn=loss_fn, grnd_eval=evl.grnd_eval)
    T_max = int(rows_all["srl_arg_word_mask_len"].max())
    ex = bank(first["vid_index"], {k: first[k].cuda() for k in dls.PER_QUERY_KEYS}, with_loss_keys=False)
    ex.pop("_keepalive", None)
    ex.update({k: first[k] for k in cols if k != "vid_index"})
    slot = eng.make_slot(ex, T=T_max, graph=True)
    stg = dls.PackedStaging({"qry_index": torch.zeros(B, dtype=torch.int32), "val_step": torch.zeros(4, dtype=torch.int32)}, n_dev=1)
    assert set(stg.host) == {"qry_index", "val_step"} and stg.nbytes == 512
    slot.feed_from(stg, assembler=bank, via="device", epilogue=epi, queries=qb)
    cs = torch.cuda.Stream()

    def launch(staging, rows, step, extra=None):
        staging.host["qry_index"].copy_(torch.tensor(rows, dtype=torch.int32))
        staging.host["val_step"][0] = step
        staging.fill(extra or {})
        staging.upload_on(cs)
        slot.launch()
        staging.release()
        slot.consumed().synchronize()

    def eager(rows, over=None):
        hb = {k: v[torch.tensor(rows)] for k, v in rows_all.items()}
        hb.update(over or {})
        batch = next(iter(dls.BankLoader(bank, [hb])))
        with torch.no_grad():
            out = mdl(batch, T=T_max)
            ld = loss_fn(out, batch)
            rec = evl._records(out, batch)
            words = evl._ground_metrics(rec, batch, ncmp, int(eng.desc.nsrl), B)
        torch.cuda.synchronize()
        return ld, rec, words

    picks = {3: [7, 2, 17, 12], 0: [19, 18, 1, 0], 4: [5, 5, 9, 14]}
    assert B == 4
    for step, rows in picks.items():
        launch(stg, rows, step)
    slot.check()
    log.check()
    assert log.written.cpu().tolist() == [1, 0, 0, 1, 1]
    for step, rows in picks.items():
        assert np.array_equal(qb.meta(rows)["sent_idx"], rows_all["sent_idx"].numpy()[rows])
        ld, rec, words = eager(rows)
        assert torch.equal(log.loss[step, 0].view(torch.int32), ld["loss"].view(torch.int32)), step
        assert torch.equal(log.loss[step, 1].view(torch.int32), ld["mdl_out_loss"].view(torch.int32)), step
        assert torch.equal(log.words[step], words), step
        assert torch.equal(log.rec[step].view(torch.int32), rec.reshape(-1).view(torch.int32)), step
    assert bool((log.words[[3, 0, 4]] != 0).any()) and not torch.equal(log.rec[3], log.rec[0])
    # the override rule: `target_cmp` staged with other values than the column's
    stg2 = dls.PackedStaging({"qry_index": torch.zeros(B, dtype=torch.int32), "val_step": torch.zeros(4, dtype=torch.int32),
                              "target_cmp": torch.zeros(B, dtype=torch.int64)}, n_dev=1)
    slot.feed_from(stg2, assembler=bank, via="device", epilogue=epi, queries=qb)
    rows = picks[3]
    other = (rows_all["target_cmp"][torch.tensor(rows)] + 1) % ncmp
    launch(stg2, rows, 1, {"target_cmp": other})
    slot.check()
    ld, rec, words = eager(rows, {"target_cmp": other})
    assert torch.equal(log.loss[1, 0].view(torch.int32), ld["loss"].view(torch.int32))
    assert torch.equal(log.words[1], words) and torch.equal(log.rec[1].view(torch.int32), rec.reshape(-1).view(torch.int32))
    assert not torch.equal(log.loss[1, 0], log.loss[3, 0])                  # (the column's values give another loss)
    assert torch.equal(slot.inp["target_cmp"].cpu(), other)


# ---- 4: Evaluator.forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("small/vog_spat", None), ("small/vog_spat", "f32"), ("small/vog_svsq", "f16")])
def test_evaluator_query_bank_equals_val_graph_and_the_existing_loop(name, dtype, tmp_path, tmp_path_factory):
    """19 batches of 4, the last a query short, from a host loader (dtype None) and from bank loaders: val_graph + query_bank,
    val_graph alone and the existing loop return equal losses, metrics and pickle bytes; the staging buffer shrinks."""
    cfg, sd, comm, sel, dl = _eval_set(name, tmp_path_factory)
    assert len(dl) == 19 and int(dl[-1]["num_cmp_msk"].shape[0]) == 3
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    if dtype is None:
        loader = lambda: dl
    else:
        bank, index_batches = _bank_and_index_batches(cfg, comm, dl, dtype)
        loader = lambda: bank.loader(index_batches)
    for i, hip in enumerate(COMBOS):
        ref = _run(cfg, mdl, evl, loss_fn, loader(), tmp_path / f"e{i}", query_bank=False, **hip)
        vg = _run(cfg, mdl, evl, loss_fn, loader(), tmp_path / f"g{i}", val_graph=True, query_bank=False, **hip)
        st_vg = dict(evl.val_graph_stats)
        got = _run(cfg, mdl, evl, loss_fn, loader(), tmp_path / f"q{i}", val_graph=True, query_bank=True, **hip)
        st_qb = dict(evl.val_graph_stats)
        _assert_same(ref, vg, (name, dtype, hip, "val_graph"))
        _assert_same(ref, got, (name, dtype, hip, "query_bank"))
        assert (ref[2] is None) == (hip.get("val_pickle") is False) and ref[0]["loss"] > 0
        print(name, dtype, hip, "staging bytes", st_vg["staging_bytes"], "->", st_qb["staging_bytes"], "query bank", st_qb["query_bank_bytes"])
        assert st_vg["query_bank_bytes"] == 0 and st_qb["query_bank_bytes"] > 0
        assert 0 < st_qb["staging_bytes"] < st_vg["staging_bytes"]
        assert st_qb["steps"] == 19 and st_qb["graph_steps"] == 18
    cfg.hip["query_bank"] = False


# ---- 5: a weight reload between two validations -----------------------------------------------------------------------------
def test_weights_reloaded_between_two_query_bank_validations(tmp_path, tmp_path_factory):
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    first = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "q1", device_metrics=True, val_graph=True, query_bank=True)
    qb, old_pipe = evl._val_graph_cache["qbank"][1], evl._val_graph_cache["pipe"][1]
    assert old_pipe.queries is qb and all(sl.queries is qb for sl in old_pipe.slots)
    sd2 = {k: (v * np.float32(1.25) if k.startswith("lin2.") else v) for k, v in sd.items()}
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
    got = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "q2", device_metrics=True, val_graph=True, query_bank=True)
    new_pipe = evl._val_graph_cache["pipe"][1]
    assert evl._val_graph_cache["qbank"][1] is qb and new_pipe is not old_pipe and new_pipe.queries is qb
    ref = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "e2", device_metrics=True, query_bank=False)
    _assert_same(ref, got, "new weights")
    assert got[0] != first[0]
    cfg.hip["query_bank"] = False


# ---- 6: the training side ---------------------------------------------------------------------------------------------------
def test_query_loader_equals_bank_loader_and_trains_the_same(tmp_path_factory):
    """`QueryBank.loader({qry_index, vid_index, target_cmp}, bank)` against `BankLoader` on the full index batches: every key
    equal; one FP32Trainer.step on either batch returns the same loss bits."""
    trn = importlib.import_module("vognet-pytorch_amd.train")
    cfg, sd, comm, sel, dl = _eval_set("small/vog_spat", tmp_path_factory)
    bank, index_batches = _bank_and_index_batches(cfg, comm, dl, "f32")
    full = index_batches[:3]
    qb = dls.QueryBank.from_batches(full, keys=[k for k in full[0] if k != "vid_index"])
    B = int(full[0]["vid_index"].shape[0])
    rows = [[9, 0, 5, 5], [3, 11, 2, 8]]                      # any rows, not the batches' own order
    rows_all = {k: torch.cat([bt[k] for bt in full]) for k in full[0]}
    small, big = [], []
    for r in rows:
        sel_rows = torch.tensor(r)
        hb = {k: v[sel_rows] for k, v in rows_all.items()}
        hb["target_cmp"] = (hb["target_cmp"] + 1) % hb["vid_index"].shape[1]          # re-sampled per epoch: an override
        big.append(hb)
        small.append({"qry_index": torch.tensor(r, dtype=torch.int32), "vid_index": hb["vid_index"], "target_cmp": hb["target_cmp"]})
    ql = qb.loader(small, bank)
    assert len(ql) == 2 and B == 4
    a_batches, b_batches = list(ql), list(bank.loader(big))
    torch.cuda.synchronize()
    for a, b in zip(a_batches, b_batches):
        assert set(a) == set(b) and "qry_index" not in a and "vid_index" not in a
        for k in b:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    losses = []
    for batch in (a_batches[0], b_batches[0]):
        tr = trn.FP32Trainer(cfg, comm, {k: torch.from_numpy(v) for k, v in sd.items()}, sel["loss"](cfg, comm), lr=1e-4)
        losses.append(np.float32(float(tr.step(batch)["loss"])))
    torch.cuda.synchronize()
    assert losses[0].tobytes() == losses[1].tobytes() and losses[0] > 0
