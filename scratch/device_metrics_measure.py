"""Measurements behind profiles/device_metrics.md (run on the MI355X box from the repository root):

    python scratch/device_metrics_measure.py stage   OUT.json     # the metric stage alone, one set of records
    python scratch/device_metrics_measure.py forward OUT.json     # Evaluator.forward wall time, three settings, interleaved

stage: 20 000 synthetic sentences (tests/metrics_util.py generator) for spat (4 videos) and svsq (1 video, SEP rules): the host
pass `eval_ground_acc(pickle)` (what the parent commit runs; the pickle is written by fast_pickle as the evaluator does) against
kernel + device-to-host copy of the result words + host aggregation. Kernel times: events around many launches.
forward: `Evaluator.forward` on the full-size cfg 2 (vog, spat) and cfg 5 (vog, svsq) models, bsv = 4, 20 000 queries whose
annotations follow the loader (tests/test_gpu_device_metrics.py::make_eval_set; 8 feature batches shared by the 5 000 loader
batches), for (a) host metrics, (b) device metrics + pickle, (c) device metrics, no pickle; three rounds a-b-c-a-b-c-...
(`main_dist --only_val` itself runs on a loader without annotation files, so it has no metric stage to time.)"""
import ctypes as C
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import metrics_util as U                                     # noqa: E402

L = importlib.import_module("vognet-pytorch_amd.lib")
FP = importlib.import_module("vognet-pytorch_amd.fast_pickle")
N = int(os.environ.get("VOG_METRIC_SENTENCES", 20000))


def stage(conc, ncmp, tmp):
    U.NCMP = ncmp
    rows, ent = U.annotation_set(7, N)
    cfg = U.write_annotations(os.path.join(tmp, f"ann_{conc}"), rows, ent)
    rule = "sep" if conc == "svsq" else conc
    arr = U.predictions(rows, ent, rule, 71)
    ev = U.CLS[rule](cfg, {"num_prop_per_frm": 5})
    n = len(arr["idx_sent"])
    b = np.zeros(arr["pred_boxes"].shape[:-1] + (7,), dtype=np.float32)
    b[..., :5] = arr["pred_boxes"]
    cols = {"pred_boxes": b, "pred_scores": arr["pred_scores"], "pred_cmp": arr["pred_cmp"], "idx_vid": arr["idx_vid"].astype(np.int64),
            "idx_verbs": arr["idx_verbs"].astype(np.int64), "idx_sent": arr["idx_sent"].astype(np.int64),
            "cmp_msk": arr["cmp_msk"].astype(np.int64), "targ_cmp": arr["targ_cmp"].astype(np.int64),
            "perm": np.tile(np.arange(ncmp), (n, 1)).astype(np.int64), "perm_inv": np.tile(np.arange(ncmp), (n, 1)).astype(np.int64)}
    fname = os.path.join(tmp, f"{conc}.pkl")
    with open(fname, "wb") as f:
        f.write(FP.dumps_records(cols))
    res = {"conc": conc, "ncmp": ncmp, "records": n, "pickle_MB": os.path.getsize(fname) / 2 ** 20}
    t0 = time.time()
    host = ev.eval_ground_acc(fname)
    res["host_eval_ground_acc_s"] = time.time() - t0

    lib = L.load()
    rec = torch.from_numpy(U.pack_records(arr)).cuda()
    meta = [torch.from_numpy(np.ascontiguousarray(arr[k].astype(np.int64))).cuda() for k in ("idx_sent", "idx_verbs", "cmp_msk", "targ_cmp")]
    t0 = time.time()
    tab, _ = ev.device_table("cuda")
    torch.cuda.synchronize()
    res["table_build_upload_s"] = time.time() - t0
    words = torch.zeros(n, dtype=torch.int32, device="cuda")

    def args(B):
        a = L.GMetricArgs()
        a.rec = L.ptr(rec)
        a.idx_sent, a.idx_verbs, a.cmp_msk, a.targ_cmp = (L.ptr(c) for c in meta)
        a.tab, a.result = C.pointer(tab), L.ptr(words)
        a.B, a.ncmp, a.nsrl, a.nfrm0, a.conc_type, a.prob_thresh = B, ncmp, U.NSRL, U.NFRM, L.CONC_TYPE[rule], float(ev.prob_thresh)
        return a

    for B, reps in ((n, 200), (64, 2000), (4, 2000)):
        a = args(B)
        for _ in range(10):
            L.check(lib.vog_ground_metrics(C.byref(a), L.stream_ptr()))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            L.check(lib.vog_ground_metrics(C.byref(a), L.stream_ptr()))
        e1.record()
        torch.cuda.synchronize()
        res[f"kernel_us_per_launch_B{B}"] = e0.elapsed_time(e1) * 1e3 / reps
    L.check(lib.vog_ground_metrics(C.byref(args(n)), L.stream_ptr()))
    torch.cuda.synchronize()
    t0 = time.time()
    w = words.cpu().numpy()
    res["d2h_copy_s"] = time.time() - t0
    t0 = time.time()
    dev = ev.eval_ground_acc_from_results(w, arr["idx_sent"])
    res["host_aggregation_s"] = time.time() - t0
    res["equal_dictionaries"] = bool(dev == host)
    res["avg1"] = float(host["avg1"])
    res["device_stage_s"] = res[f"kernel_us_per_launch_B{n}"] * 1e-6 + res["d2h_copy_s"] + res["host_aggregation_s"]
    res["host_queries_per_s"] = n / res["host_eval_ground_acc_s"]
    res["device_queries_per_s"] = n / res["device_stage_s"]
    return res


def forward(name, tmp, rounds=3):
    T = importlib.import_module("tests.test_gpu_device_metrics")
    B = 4
    cfg, sd, comm, sel, dl = T.make_eval_set(name, os.path.join(tmp, "ann_" + name.replace("/", "_")), n_batches=(N + B) // B, B=B, distinct=8)
    pinned = {}
    for b in dl:                                                        # the shared feature tensors: pinned once
        for k, v in list(b.items()):
            if v.numel() > 4096:
                b[k] = pinned.setdefault((k, v.data_ptr(), tuple(v.shape)), v if v.is_pinned() else v.pin_memory())
    mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
    settings = {"a_host": {}, "b_device": {"device_metrics": True}, "c_device_nopickle": {"device_metrics": True, "val_pickle": False}}
    T._run(cfg, mdl, evl, loss_fn, dl, os.path.join(tmp, "warm"), device_metrics=True, val_pickle=False)    # warm-up: graphs, table, allocator
    out = {"case": name, "queries": sum(int(b["sent_idx"].shape[0]) for b in dl), "seconds": {k: [] for k in settings}, "val_acc": {}}
    for r in range(rounds):
        for k, hip in settings.items():
            torch.cuda.synchronize()
            t0 = time.time()
            acc, _, path = T._run(cfg, mdl, evl, loss_fn, dl, os.path.join(tmp, f"{k}{r}"), **hip)
            out["seconds"][k].append(time.time() - t0)
            out["val_acc"].setdefault(k, acc)
            assert acc == out["val_acc"]["a_host"], (k, acc, out["val_acc"]["a_host"])
            assert path == ("host" if k == "a_host" else "device")
            f = os.path.join(tmp, f"{k}{r}", "valid_0.pkl")
            if os.path.isfile(f):
                os.remove(f)
    out["median_s"] = {k: float(np.median(v)) for k, v in out["seconds"].items()}
    return out


if __name__ == "__main__":
    mode, dst = sys.argv[1], sys.argv[2]
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        if mode == "stage":
            for conc, ncmp in (("spat", 4), ("svsq", 1)):
                results.append(stage(conc, ncmp, tmp))
                print(json.dumps(results[-1]), flush=True)
        else:
            for name in sys.argv[3:] or ["full/cfg2_vog_spat_gt5_bs4", "full/cfg5_vog_svsq_gt5_bs16"]:
                results.append(forward(name, tmp))
                print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(results, f, indent=1)
