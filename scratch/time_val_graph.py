"""What `cfg.hip.val_graph` buys the validation loop (writes profiles/val_graph.json; bench.py is untouched).

    python scratch/time_val_graph.py [--queries 20000] [--rounds 3] [--videos 4096] [--cases cfg2,cfg5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scratch/time_val_graph.py --trace-only --queries 2000   # kernel times, own run
    python scratch/time_val_graph.py --merge-stats DIR                                                      # -> the json's "epilogue_kernels"

One process, per case (full-size cfg 2 spat, cfg 5 svsq; bsv = 4; an f16 FeatureBank; device metrics on; with and without the
prediction pickle) three loops ALTERNATED round by round after an untimed run of each (other people's work shares the host: a
difference only counts against the spread of a loop's own rounds):
  (a) existing   Evaluator.forward on bank.loader(index batches): the loop the parent commit runs
  (b) val_graph  the same call with cfg.hip.val_graph = True
  (c) ceiling    the forward-only bank-fed engine.FedPipeline loop over the same index batches (no loss, metrics or log)
queries/s = queries / seconds, host clock around a call that ends in a synchronise. (b) also reports the host's time per batch
inside its loop (Evaluator.val_graph_stats). The annotation set follows the loader as in tests/test_gpu_device_metrics.py;
the bank's videos are synthetic, so the metrics themselves mean nothing here - (a) and (b) must still return the same ones.
"""
from __future__ import annotations

import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "val_graph.json")
CASES = {"cfg2": "full/cfg2_vog_spat_gt5_bs4", "cfg5": "full/cfg5_vog_svsq_gt5_bs16"}
EPILOGUE = ("loss_partial_kernel", "loss_finish_kernel", "ground_metrics_kernel", "ground_metrics_log_kernel", "val_log_kernel")
LANG_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
             "srl_arg_inds_msk", "num_cmp_msk")


def merge_stats(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    res = json.load(open(OUT))
    got = {}
    for name in EPILOGUE + ("bank_rows_kernel", "copy_segments_kernel"):
        hit = [r for r in rows if name in r.get("Name", "")]
        if hit:
            got[name] = {"calls": sum(int(r["Calls"]) for r in hit), "avg_us": sum(float(r["AverageNs"]) * int(r["Calls"]) for r in hit) / sum(int(r["Calls"]) for r in hit) / 1e3}
    # a graph step's launches: the kernels nearly every step ran (the stand-alone forms of the tail batches are listed, not summed)
    most = max(v["calls"] for k, v in got.items() if k in EPILOGUE)
    got["epilogue_us_per_step"] = sum(v["avg_us"] for k, v in got.items() if k in EPILOGUE and 2 * v["calls"] > most)
    got["epilogue_launches_per_step"] = sum(1 for k, v in got.items() if k in EPILOGUE and 2 * v["calls"] > most)
    got["source"] = "rocprofv3 --kernel-trace --stats, a run of its own (loop (b) only, cfg 2, pickle on)"
    res["epilogue_kernels"] = got
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(got))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--videos", type=int, default=4096)
    ap.add_argument("--cases", default="cfg2,cfg5")
    ap.add_argument("--trace-only", action="store_true", help="loop (b) alone on cfg 2, for a rocprofv3 run; writes nothing")
    ap.add_argument("--merge-stats", metavar="DIR")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats)

    import numpy as np
    import torch
    T = importlib.import_module("tests.test_gpu_device_metrics")
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    eng_mod = importlib.import_module("vognet-pytorch_amd.engine")
    dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: there is no fallback, and a CPU run says nothing about these rates")
    torch.cuda.set_device(0)
    B = 4
    allres = json.load(open(OUT)) if os.path.isfile(OUT) else {}

    def run(cfg, mdl, evl, loss_fn, dl, out_dir, **hip):
        for k, v in {"device_metrics": True, "val_pickle": True, "batch_requests": 1, "val_graph": False, **hip}.items():
            cfg.hip[k] = v
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            loss, acc = evl(mdl, loss_fn, dl, "valid", rank=0, pred_path=out_dir)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        f = os.path.join(str(out_dir), "valid_0.pkl")
        if os.path.isfile(f):
            os.remove(f)
        return dt, {k: float(v) for k, v in loss.items()}, {k: float(v) for k, v in acc.items()}

    def summary(v):
        med = statistics.median(v)
        return {"queries_per_s_median": med, "queries_per_s_min": min(v), "queries_per_s_max": max(v), "spread": (max(v) - min(v)) / med,
                "us_per_batch_median": B / med * 1e6, "rounds": v}

    for key in ([c for c in args.cases.split(",") if c] if not args.trace_only else ["cfg2"]):
        name = CASES[key]
        with tempfile.TemporaryDirectory() as tmp:
            n_batches = (args.queries + B) // B                      # (the last batch is a query short)
            cfg, sd, comm, sel, dl = T.make_eval_set(name, os.path.join(tmp, "ann"), n_batches=n_batches, B=B, distinct=8)
            nq = sum(int(b["sent_idx"].shape[0]) for b in dl)
            nppf0 = comm["num_prop_per_frm"]
            bank = dls.FeatureBank(cfg, comm, args.videos, dtype="f16")
            chunk = min(256, args.videos)
            it = synth.make_items(chunk, 1, nppf0, seed=3)
            one = {k: np.ascontiguousarray(it[k][:, 0]) for k in dls.BANK_KEYS}
            for s0 in range(0, args.videos, chunk):
                n = min(chunk, args.videos - s0)
                bank.put(s0, {k: v[:n] for k, v in one.items()})
            drop = set(dls.BANK_KEYS) | {"pad_frm_mask"}
            rng = np.random.default_rng(0)
            index_batches = []
            for hb in dl:
                b, ncmp = hb["num_cmp_msk"].shape
                index_batches.append({**{k: v for k, v in hb.items() if k not in drop},
                                      "vid_index": torch.from_numpy(rng.integers(0, args.videos, size=(b, ncmp)).astype(np.int32))})
            del dl
            mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
            eng = mdl.engine()
            assert bank.lossless_for(eng), eng.plan

            if args.trace_only:
                run(cfg, mdl, evl, loss_fn, bank.loader(index_batches), os.path.join(tmp, "w"), val_graph=True)
                dt, _, _ = run(cfg, mdl, evl, loss_fn, bank.loader(index_batches), os.path.join(tmp, "t"), val_graph=True)
                print(f"trace run: val_graph {nq / dt:.0f} queries/s (under the tracer: not a result)")
                return

            # (c) the forward-only bank-fed loop over the same index batches
            first = index_batches[0]
            T_max = max(int(b["srl_arg_word_mask_len"].max()) for b in index_batches)
            lang = [k for k in LANG_KEYS + (("verb_ind_in_srl",) if eng.sep else ())]
            ex = bank(first["vid_index"], with_loss_keys=False)
            ex.pop("_keepalive", None)
            ex.update({k: first[k] for k in lang})
            spec = {"vid_index": first["vid_index"], **{k: first[k] for k in lang}}
            pipe_c = eng_mod.FedPipeline(eng, ex, spec, bank, streams=4, slots_per_stream=2, T=T_max)
            full = [b for b in index_batches if int(b["vid_index"].shape[0]) == B]

            def loop_c():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for hb in full:
                    st = pipe_c.next_staging()
                    st.host["vid_index"].copy_(hb["vid_index"])
                    for k in lang:
                        st.host[k].copy_(hb[k])
                    pipe_c.submit()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            res = {"case": name, "queries": nq, "bsv": B, "plan": eng.plan, "bank": {"videos": args.videos, "dtype": "f16"},
                   "rounds": args.rounds, "settings": {}}
            for tag, hip in (("pickle", {}), ("no_pickle", {"val_pickle": False})):
                rates = {"existing": [], "val_graph": [], "ceiling": []}
                host_us = []
                ref, equal = None, True
                for r in range(args.rounds + 1):                      # round 0: untimed
                    dt_a, loss_a, acc_a = run(cfg, mdl, evl, loss_fn, bank.loader(index_batches), os.path.join(tmp, f"a{tag}{r}"), **hip)
                    dt_b, loss_b, acc_b = run(cfg, mdl, evl, loss_fn, bank.loader(index_batches), os.path.join(tmp, f"b{tag}{r}"), val_graph=True, **hip)
                    assert evl.val_path == "graph"
                    st = dict(evl.val_graph_stats)
                    dt_c = loop_c()
                    ref = ref or (loss_a, acc_a)
                    equal = equal and (loss_b, acc_b) == ref and (loss_a, acc_a) == ref
                    if r == 0:
                        continue
                    rates["existing"].append(nq / dt_a)
                    rates["val_graph"].append(nq / dt_b)
                    rates["ceiling"].append(len(full) * B / dt_c)
                    host_us.append(st["host_s"] / st["steps"] * 1e6)
                s = {k: summary(v) for k, v in rates.items()}
                s["val_graph_host_us_per_batch"] = statistics.median(host_us)
                s["staging_bytes_per_query"] = st["staging_bytes"] / B
                s["val_graph_over_existing"] = s["val_graph"]["queries_per_s_median"] / s["existing"]["queries_per_s_median"]
                s["val_graph_range_wholly_above_existing"] = s["val_graph"]["queries_per_s_min"] > s["existing"]["queries_per_s_max"]
                s["val_graph_fraction_of_ceiling"] = s["val_graph"]["queries_per_s_median"] / s["ceiling"]["queries_per_s_median"]
                s["val_loss"], s["val_acc"] = ref
                s["both_loops_return_the_same_loss_and_metrics"] = equal
                res["settings"][tag] = s
                print(key, tag, json.dumps({k: round(v["queries_per_s_median"]) for k, v in s.items() if isinstance(v, dict) and "rounds" in v}),
                      "host us/batch", round(s["val_graph_host_us_per_batch"], 1), "above:", s["val_graph_range_wholly_above_existing"], "equal:", equal, flush=True)
            bank.check()
            allres[key] = res
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            json.dump(allres, open(OUT, "w"), indent=1)
            del pipe_c, evl, mdl, bank
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
