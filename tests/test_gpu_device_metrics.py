"""Grounding metrics on the device (csrc/metrics.hip, `vog_ground_metrics`) against the host rules of eval_fn_corr.py.

The kernel returns one word of counts per prediction record; the host `eval_one_sent_idx` of the same record, packed the
same way, is the reference: the words must be EQUAL (the rules are discrete, the IoU is reproduced operation for operation).
Sets: the reference-generated fixtures of tests/golden/metrics/ (aggregated dictionaries pinned by expected.json), larger
random sets with hostile cases from tests/metrics_util.py, and `Evaluator.forward` end to end with `cfg.hip.device_metrics`
/ `cfg.hip.val_pickle`, on one and on two ranks."""
import ctypes as C
import importlib
import json
import os
import socket

import numpy as np
import pytest
import torch

from tests import metrics_util as U

pytestmark = pytest.mark.gpu

L = importlib.import_module("vognet-pytorch_amd.lib")
M = U.M


def run_kernel(ev, arr, conc, stream=None, out=None, nsrl=None):
    """vog_ground_metrics on the records of `arr` -> (int32 words on the host, the device buffers)."""
    lib = L.load()
    rec = torch.from_numpy(U.pack_records(arr)).cuda()
    B, ncmp = arr["cmp_msk"].shape
    nsrl = nsrl or arr["pred_scores"].shape[1]
    nfrm = arr["pred_scores"].shape[3]
    assert rec.shape[1] * 4 == lib.vog_pred_record_bytes(ncmp, nsrl, nfrm)
    cols = [torch.from_numpy(np.ascontiguousarray(arr[k].astype(np.int64))).cuda() for k in ("idx_sent", "idx_verbs", "cmp_msk", "targ_cmp")]
    tab, _ = ev.device_table("cuda")
    res = out if out is not None else torch.full((B,), -1, dtype=torch.int32, device="cuda")
    a = L.GMetricArgs()
    a.rec = L.ptr(rec)
    a.idx_sent, a.idx_verbs, a.cmp_msk, a.targ_cmp = (L.ptr(c) for c in cols)
    a.tab = C.pointer(tab)
    a.result = L.ptr(res)
    a.B, a.ncmp, a.nsrl, a.nfrm0, a.conc_type, a.prob_thresh = B, ncmp, nsrl, nfrm, L.CONC_TYPE[conc], float(ev.prob_thresh)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        L.check(lib.vog_ground_metrics(C.byref(a), L.stream_ptr(s)), "vog_ground_metrics")
    s.synchronize()
    return res.cpu().numpy(), (rec, cols, res)


def describe(w):
    return dict(res=int(w & 15), tot=int((w >> 4) & 15), cons=int((w >> 8) & 1), vidf=int((w >> 9) & 1), strict=int((w >> 10) & 1),
                err=int(w >> 16))


def assert_words_equal(got, want, what):
    bad = np.nonzero(got != want)[0]
    msg = [f"record {i}: device {describe(got[i])} host {describe(want[i])}" for i in bad[:8]]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} result words differ\n" + "\n".join(msg)


# ---- the reference-generated fixtures -------------------------------------------------------------------------------------
@pytest.mark.parametrize("conc", ["sep", "temp", "spat"])
def test_kernel_matches_host_and_reference_on_fixtures(conc):
    ev = U.CLS[conc](U.cfg_for(), {"num_prop_per_frm": 5})
    arr = U.fixture_arrays(conc)
    want = U.host_words(ev, U.records(arr, conc))
    got, _ = run_kernel(ev, arr, conc)
    assert_words_equal(got, want, conc)
    out = ev.eval_ground_acc_from_results(got, arr["idx_sent"])
    exp = json.load(open(os.path.join(U.GOLD, "expected.json")))[conc]
    for k in U.KEYS:
        if k in exp:
            assert out[k] == pytest.approx(exp[k], rel=0, abs=1e-12), (conc, k)
    assert set(out["classwise_dict"]) == set(exp["classes"])
    for verb, per_q in out["classwise_dict"].items():
        idx = sorted(per_q)
        flat = [float(per_q[i][r]) for r in ev.res_dicts for i in idx] + [float(per_q[i]["tot_dict"]) for i in idx]
        assert flat == exp["classes"][verb], (conc, verb)


# ---- the IoU ------------------------------------------------------------------------------------------------------------------
def test_iou_is_bit_exact():
    """vog_box_iou_f32 (the metric kernel's arithmetic) against box_iou_f32: the same bits, hence the same `> 0.5`."""
    rng = np.random.RandomState(5)
    n = 6000
    x1, y1 = rng.randint(0, 2880, n), rng.randint(0, 480, n)
    a = np.stack([x1, y1, x1 + rng.randint(0, 300, n), y1 + rng.randint(0, 200, n)], axis=1).astype(np.float32)
    b = a + rng.randint(-40, 41, (n, 4)).astype(np.float32)            # overlapping pairs around every IoU, some inverted
    b[:1500] = np.stack([rng.randint(0, 2880, 1500), rng.randint(0, 480, 1500), rng.randint(0, 2880, 1500), rng.randint(0, 480, 1500)], axis=1)
    frac = (rng.rand(1000, 4) * 720).astype(np.float32)                  # non-integer predictions
    a[1500:2500] = np.sort(frac.reshape(1000, 2, 2), axis=1).reshape(1000, 4)
    b[1500:2500] = np.round(a[1500:2500]) + rng.randint(-3, 4, (1000, 4))
    hard_a = [[0, 0, 10, 10], [0, 0, 10, 10], [5, 5, 5, 5], [0, 0, 0, 0], [3, 4, 50, 60], [0, 0, 10, 10], [2870, 0, 2880, 10],
              [2160, 100, 2879, 479], [0, 0, 30, 30], [0, 0, 3, 1], [2161, 7, 2878, 333], [0, 0, 20, 10], [100, 100, 90, 90]]
    hard_b = [[0, 0, 10, 5], [5, 0, 15, 10], [5, 5, 5, 5], [0, 0, 0, 0], [3, 4, 50, 60], [20, 20, 30, 30], [2870, 0, 2880, 5],
              [2160, 100, 2879, 290], [0, 0, 30, 10], [0, 0, 2, 1], [2161, 7, 2878, 170], [0, 0, 10, 10], [80, 80, 120, 120]]
    # thirds: inter / union = 1/3 in exact arithmetic, 0.5 +- one ulp candidates from scaled copies of the IoU-0.5 pair
    for k in range(1, 400):
        hard_a.append([0, 0, 2 * k, k + 7]); hard_b.append([0, 0, k, k + 7])
        hard_a.append([720 * 3 + k, k, 720 * 3 + 3 * k + 1, 3 * k + 2]); hard_b.append([720 * 3 + k, k, 720 * 3 + 3 * k + 1, 2 * k + 1])
    a = np.concatenate([a, np.asarray(hard_a, np.float32)])
    b = np.concatenate([b, np.asarray(hard_b, np.float32)])
    want = np.array([M.box_iou_f32(x, y) for x, y in zip(a, b)], dtype=np.float32)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.empty(len(a), dtype=torch.float32, device="cuda")
    L.check(L.load().vog_box_iou_f32(L.ptr(da), L.ptr(db), L.ptr(out), len(a), L.stream_ptr()), "vog_box_iou_f32")
    got = out.cpu().numpy()
    assert np.isnan(want).sum() >= 2 and (want == 0.5).sum() >= 100 and (want == 1).sum() >= 1 and (want == 0).sum() >= 100
    assert ((want > 0.5) & (want < 0.6)).sum() >= 50 and ((want < 0.5) & (want > 0.4)).sum() >= 50
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), [(a[i].tolist(), b[i].tolist(), float(got[i]), float(want[i])) for i in np.nonzero(~same)[0][:5]]
    assert np.array_equal(got > 0.5, want > 0.5)


# ---- random sets with hostile cases --------------------------------------------------------------------------------------------
_SETS = {}


def _annotations(seed, tmp_path_factory):
    if seed not in _SETS:
        rows, ent = U.annotation_set(seed, 2000)
        d = tmp_path_factory.mktemp(f"ann{seed}")
        _SETS[seed] = (rows, ent, U.write_annotations(str(d), rows, ent))
    return _SETS[seed]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("conc", ["sep", "temp", "spat"])
def test_kernel_matches_host_on_random_sets(conc, seed, tmp_path_factory):
    """2000 sentences per set: every result word equals the host's. The set is checked to be non-degenerate first."""
    rows, ent, cfg = _annotations(seed, tmp_path_factory)
    arr = U.predictions(rows, ent, conc, 10 * seed + {"sep": 1, "temp": 2, "spat": 3}[conc])
    ev = U.CLS[conc](cfg, {"num_prop_per_frm": 5})
    recs = U.records(arr, conc)
    want = U.host_words(ev, recs)
    host = ev.eval_ground_acc_from_results(want, arr["idx_sent"])
    scored = want[((want >> 4) & 15) > 0]
    hostile = U.hostile_counts(ev, recs, conc)
    print(conc, seed, {k: round(float(host[k]), 3) for k in ("avg1", "avg1_cons", "avg1_vidf", "avg1_strict")}, hostile)
    assert 0.1 <= host["avg1"] <= 0.9
    assert set(np.unique((scored >> 10) & 1)) == {0, 1}
    if conc != "sep":                                                  # (sep's cons is 1 by definition)
        assert set(np.unique((scored >> 8) & 1)) == {0, 1} and set(np.unique((scored >> 9) & 1)) == {0, 1}
    assert (want == 0).sum() > 0 and int(((want >> 4) & 15).max()) > 5 # sentences without groundable arguments / with some past nsrl
    need = ["thresh_equal", "multi_box_frame", "repeated_frame"] + (["tied_cmp"] if conc == "sep" else ["tied_best"])
    assert all(hostile[k] > 0 for k in need), hostile
    got, _ = run_kernel(ev, arr, conc)
    assert_words_equal(got, want, f"{conc} seed {seed}")
    assert ev.eval_ground_acc_from_results(got, arr["idx_sent"]) == host


@pytest.mark.parametrize("conc", ["sep", "temp", "spat"])
def test_kernel_matches_host_beyond_one_wave_of_lanes(conc, tmp_path, monkeypatch):
    """Shapes at which every lane loop of the kernel runs more than once: 70 frames, 3 x 70 entries of pred_cmp, segments of
    up to 150 boxes and arguments with up to 100 of them (64 lanes per pass)."""
    monkeypatch.setattr(U, "NFRM", 70)
    monkeypatch.setattr(U, "NSRL", 3)
    monkeypatch.setattr(U, "NCMP", 3)
    rows, ent = U.annotation_set(5, 300, max_box=150, max_k=100)
    cfg = U.write_annotations(str(tmp_path), rows, ent)
    cfg.ds.num_sampled_frm = 70
    arr = U.predictions(rows, ent, conc, 55)
    ev = U.CLS[conc](cfg, {"num_prop_per_frm": 5})
    t = ev.host_table()
    assert t["box_cnt"].max() > 128 and t["ind_cnt"].max() > 64
    want = U.host_words(ev, U.records(arr, conc))
    scored = want[((want >> 4) & 15) > 0]
    assert len(set((scored & 15).tolist())) > 1                       # some arguments right, some wrong
    got, _ = run_kernel(ev, arr, conc)
    assert_words_equal(got, want, conc)


def test_error_bits_raise_what_the_host_raises():
    conc = "spat"
    ev = U.CLS[conc](U.cfg_for(), {"num_prop_per_frm": 5})
    arr = {k: v[:8].copy() for k, v in U.fixture_arrays(conc).items()}
    arr["idx_verbs"][1, arr["targ_cmp"][1]] = (arr["idx_sent"][1] + 1) % 64     # not the query's sentence
    arr["idx_verbs"][2, 0] = 10 ** 6 if arr["targ_cmp"][2] != 0 else arr["idx_verbs"][2, 0]
    arr["idx_verbs"][2, 1] = 10 ** 6 if arr["targ_cmp"][2] == 0 else arr["idx_verbs"][2, 1]
    arr["cmp_msk"][3, :] = 0                                                       # every chosen video is masked out
    arr["targ_cmp"][4] = 9
    got, _ = run_kernel(ev, arr, conc)
    assert got[0] >> 16 == 0 and got[5] >> 16 == 0
    assert got[1] == ev.ERR_VERB and got[2] == ev.ERR_RANGE and got[3] == ev.ERR_MASK and got[4] == ev.ERR_RANGE
    recs = U.records(arr, conc)
    with pytest.raises(AssertionError):
        ev.eval_one_sent_idx(recs[3], recs[3]["idx_sent"])
    with pytest.raises(IndexError):
        ev.eval_one_sent_idx(recs[2], recs[2]["idx_sent"])
    for i, exc in ((1, AssertionError), (2, IndexError), (3, AssertionError)):
        full = {k: v.copy() for k, v in U.fixture_arrays(conc).items()}
        words = U.host_words(ev, U.records(full, conc))
        pos = int(np.nonzero(full["idx_sent"] == 5)[0][0])            # sentence 5 is a validation row
        words[pos] = got[i]
        with pytest.raises(exc, match=f"record {pos} "):
            ev.eval_ground_acc_from_results(words, full["idx_sent"])


def test_non_default_stream_and_buffer_reuse():
    """The launch goes to the stream it is given and keeps no state: a second launch into the same result buffer with other
    records gives those records' words; a relaunch of the first gives the first words again."""
    ev = U.CLS["temp"](U.cfg_for(), {"num_prop_per_frm": 5})
    arr = U.fixture_arrays("temp")
    half = {k: v[:32] for k, v in arr.items()}
    other = {k: v[32:64] for k, v in arr.items()}
    want = U.host_words(ev, U.records(arr, "temp"))
    st = torch.cuda.Stream()
    buf = torch.full((32,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a, _ = run_kernel(ev, half, "temp", stream=st, out=buf)
    b, _ = run_kernel(ev, other, "temp", stream=st, out=buf)
    c, _ = run_kernel(ev, half, "temp", stream=st, out=buf)
    assert_words_equal(a, want[:32], "first launch")
    assert_words_equal(b, want[32:64], "second launch, same buffers")
    assert_words_equal(c, want[:32], "relaunch")
    assert not np.array_equal(a, b)


# ---- Evaluator.forward ---------------------------------------------------------------------------------------------------------
def _setup(name):
    from oracle import cases
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    cfg, sd, batch, c = cases.build(name)
    comm = {"vocab_size": c["vocab"], "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1}, "num_prop_per_frm": c["nppf0"]}
    return cfg, sd, c, comm, sel_mod.get_mdl_loss_eval(cfg), synth


def make_eval_set(name, directory, n_batches=5, B=4, distinct=None):
    """Loader batches (the last one a query short) and annotation files that follow them: sentence = running query number,
    new_srl_idxs[b, target_cmp[b]] = that sentence. The annotated boxes are copies of (integer-rounded) proposals of the target
    video: argument 0 gets ALL proposals of one frame (hit whenever the frame's score clears the threshold), argument 1 one
    proposal of another frame (hit when it is the arg-max); every other query of a multi-video set keeps only its target
    unmasked, so that SPAT's foreign-video rule cannot fail there. Host avg1 therefore lies strictly inside (0, 1).
    `distinct`: cycle through that many feature batches (large sets: the features are shared, the metadata is not)."""
    cfg, sd, c, comm, sel, synth = _setup(name)
    conc, nppf, nfrm = cfg.ds.conc_type, c["nppf0"], synth.NFRM0
    rng = np.random.RandomState(17)
    dl, rows, ent, base = [], [], {}, {}
    n_sent = n_batches * B - 1
    for i in range(n_batches):
        key = i % (distinct or n_batches)
        if key not in base:
            b = synth.make_batch(conc, B, nppf, ncmp=c["ncmp"], vocab_size=c["vocab"], prop_dim=cfg.mdl.prop_feat_dim,
                                 seg_dim=cfg.mdl.seg_feat_dim, seed=900 + key)
            b["pad_proposals"][..., :4] = np.round(b["pad_proposals"][..., :4])
            b.update(synth.make_targets(b, conc, nppf, seed=key))
            base[key] = (b, {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()})
        b, shared = base[key]
        ncmp = b["num_cmp_msk"].shape[1]
        sent = np.arange(i * B, (i + 1) * B, dtype=np.int64)
        verbs = (sent[:, None] + 1 + np.arange(ncmp)[None, :]) % n_sent
        verbs[np.arange(B), b["target_cmp"]] = sent
        msk = np.ones((B, ncmp), np.int64)
        for q in range(0, B, 2):
            msk[q] = 0
            msk[q, b["target_cmp"][q]] = 1
        own = {"ann_idx": sent.copy(), "sent_idx": sent, "new_srl_idxs": verbs, "num_cmp_msk": msk,
               "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
        for q in range(B):
            t = int(b["target_cmp"][q])
            if conc == "spat":
                pv = b["pad_proposals"][q].reshape(nfrm, ncmp, nppf, 7)[:, t].copy()
                pv[..., 0] -= 720 * t
                pv[..., 2] -= 720 * t
            else:
                pv = b["pad_proposals"][q].reshape(ncmp, nfrm, nppf, 7)[t]
            f0, f1 = rng.choice(nfrm, size=2, replace=False)
            boxes = [pv[f0, p, :4].astype(int).tolist() for p in range(nppf)] + [pv[f1, int(rng.randint(nppf)), :4].astype(int).tolist()]
            s = int(sent[q])
            ent[f"v_{s:05d}"] = {"segments": {"0": {"bbox": boxes, "frm_idx": [int(f0)] * nppf + [int(f1)]}}}
            real = b["srl_arg_inds_msk"][q].reshape(-1, b["srl_arg_inds_msk"].shape[-1])[0]
            pats = [("ARG0", int(real[0]), list(range(nppf))), ("ARG1", int(real[1]), [nppf]), ("V", 0, [0])]
            rows.append({"vt_split": "val", "ann_ind": s, "vid_seg": f"v_{s:05d}_segment_00", "lemma_verb": U.VERBS[s % 3],
                         "req_args": str([p[0] for p in pats]), "req_cls_pats_mask": str(pats)})
        t = dict(shared, **{k: torch.from_numpy(v) for k, v in own.items()})
        if i == n_batches - 1:
            t = {k: v[: B - 1] for k, v in t.items()}
        dl.append(t)
    U.write_annotations(str(directory), rows[:n_sent], {k: v for k, v in list(ent.items())[:n_sent]})
    cfg.ds.val_ds4_inds = os.path.join(str(directory), "val_asrl_annots.csv")
    cfg.ds.anet_ent_annot_file = os.path.join(str(directory), "anet_ent.json")
    cfg.train.prob_thresh = 1e-6
    cfg.train.bsv = B
    return cfg, sd, comm, sel, dl


def _evaluator(cfg, sd, comm, sel):
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return mdl, sel["eval"](cfg, comm, torch.device("cuda", 0)), sel["loss"](cfg, comm)


def _run(cfg, mdl, evl, loss_fn, dl, out_dir, **hip):
    for k, v in {"device_metrics": False, "val_pickle": True, "batch_requests": 1, **hip}.items():
        cfg.hip[k] = v
    with torch.no_grad():
        _, acc = evl(mdl, loss_fn, dl, "valid", rank=0, pred_path=out_dir)
    torch.cuda.synchronize()
    f = os.path.join(str(out_dir), "valid_0.pkl")
    return {k: float(v) for k, v in acc.items()}, (open(f, "rb").read() if os.path.isfile(f) else None), evl.metrics_path


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_svsq"])
def test_evaluator_forward_device_metrics(name, tmp_path):
    cfg, sd, comm, sel, dl = make_eval_set(name, tmp_path / "ann")
    mdl, evl, loss_fn = _evaluator(cfg, sd, comm, sel)
    assert evl.grnd_eval is not None
    host, pkl_host, path = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "a")
    assert path == "host" and set(host) == set(evl.met_keys)
    print(name, host)
    assert 0 < host["avg1"] < 1
    dev, pkl_dev, path = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "b", device_metrics=True)
    assert path == "device" and dev == host
    assert pkl_dev is not None and pkl_dev == pkl_host
    nop, pkl_none, path = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "c", device_metrics=True, val_pickle=False)
    assert path == "device" and nop == host and pkl_none is None and not (tmp_path / "c").exists()
    # two loader batches per forward, the short batch inside the last group
    host2, pkl_host2, _ = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "d", batch_requests=2)
    dev2, pkl_dev2, _ = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "e", batch_requests=2, device_metrics=True)
    nop2, _, _ = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "f", batch_requests=2, device_metrics=True, val_pickle=False)
    assert dev2 == host2 and nop2 == host2 and pkl_dev2 == pkl_host2 and 0 < host2["avg1"] < 1
    with pytest.raises(ValueError, match="val_pickle"):
        _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "g", val_pickle=False)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, name, tmp, val_pickle, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    D = importlib.import_module("vognet-pytorch_amd.dist")
    cfg, sd, comm, sel, dl = make_eval_set(name, os.path.join(tmp, f"ann{rank}"))
    mdl, evl, loss_fn = _evaluator(cfg, sd, comm, sel)
    idx = list(D.shard_indices(len(dl), rank, world))
    if (len(dl) - 1) in idx:                                            # a loader yields its short tail batch last
        idx = [i for i in idx if i != len(dl) - 1] + [len(dl) - 1]
    cfg.hip.device_metrics, cfg.hip.val_pickle = True, val_pickle
    with torch.no_grad():
        _, acc = evl(mdl, loss_fn, [dl[i] for i in idx], "valid", rank=rank, pred_path=os.path.join(tmp, "pred"))
    torch.cuda.synchronize()
    if rank == 0:
        q.put({k: float(v) for k, v in acc.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("val_pickle", [True, False])
def test_two_ranks_give_the_single_rank_metrics(tmp_path, val_pickle):
    """Two ranks on the one GPU (gloo): 4-byte result words and the host metadata meet on rank 0, rank-major; the wrapped-
    around duplicate batch of the padded shard loses to its first copy. Rank 0's val_acc equals the single-rank one."""
    import torch.multiprocessing as mp
    name, world = "small/vog_spat", 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rank_worker, args=(r, world, port, name, str(tmp_path), val_pickle, q)) for r in range(world)]
    for p in ps:
        p.start()
    got = q.get(timeout=300)
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert (tmp_path / "pred" / "valid_0.pkl").is_file() == val_pickle
    cfg, sd, comm, sel, dl = make_eval_set(name, tmp_path / "ann")
    mdl, evl, loss_fn = _evaluator(cfg, sd, comm, sel)
    one, _, _ = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "one", device_metrics=True)
    host, _, _ = _run(cfg, mdl, evl, loss_fn, dl, tmp_path / "host")
    assert got == one == host and 0 < one["avg1"] < 1
