"""What `cfg.hip.query_bank` buys the validation loop on top of `cfg.hip.val_graph` (writes profiles/query_bank.json; bench.py is
untouched). A sibling of scratch/time_val_graph.py with a fourth loop.

    python scratch/time_query_bank.py [--queries 20000] [--rounds 3] [--videos 4096] [--cases cfg2,cfg5]

One process, per case (full-size cfg 2 spat, cfg 5 svsq; bsv = 4; an f16 FeatureBank; device metrics on; with and without the
prediction pickle) four loops ALTERNATED round by round after an untimed run of each (other people's work shares the host: a
difference only counts against the spread of a loop's own rounds):
  (a) existing     Evaluator.forward on bank.loader(index batches)
  (b) val_graph    the same call with cfg.hip.val_graph = True
  (c) ceiling      the forward-only bank-fed engine.FedPipeline loop over the same index batches (no loss, metrics or log)
  (d) query_bank   (b) with cfg.hip.query_bank = True: the host writes qry_index and val_step, the graph gathers the rows
queries/s = queries / seconds, host clock around a call that ends in a synchronise, reported as median (min - max). (b) and (d)
also report the host's time per batch inside their loop (Evaluator.val_graph_stats: host_s / steps). (d) is to be compared
with (b) of the same job. The query bank is built in (d)'s untimed round and cached on the evaluator by the loader object, so
the index loader is one object for the whole case.
"""
from __future__ import annotations

import argparse
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
OUT = os.path.join(ROOT, "profiles", "query_bank.json")
CASES = {"cfg2": "full/cfg2_vog_spat_gt5_bs4", "cfg5": "full/cfg5_vog_svsq_gt5_bs16"}
LANG_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
             "srl_arg_inds_msk", "num_cmp_msk")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--videos", type=int, default=4096)
    ap.add_argument("--cases", default="cfg2,cfg5")
    args = ap.parse_args()

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
        for k, v in {"device_metrics": True, "val_pickle": True, "batch_requests": 1, "val_graph": False, "query_bank": False, **hip}.items():
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

    for key in [c for c in args.cases.split(",") if c]:
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
            # (d) runs on an evaluator of its own: an evaluator keeps ONE fed pipeline, and (b) and (d) need different ones
            evl_d = sel["eval"](cfg, comm, torch.device("cuda", 0))
            eng = mdl.engine()
            assert bank.lossless_for(eng), eng.plan

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

            loader = bank.loader(index_batches)               # ONE loader object: the evaluator caches the query bank by it
            res = {"case": name, "queries": nq, "bsv": B, "plan": eng.plan, "bank": {"videos": args.videos, "dtype": "f16"},
                   "rounds": args.rounds, "settings": {}}
            for tag, hip in (("pickle", {}), ("no_pickle", {"val_pickle": False})):
                rates = {"existing": [], "val_graph": [], "ceiling": [], "query_bank": []}
                host_us, host_us_d = [], []
                ref, equal = None, True
                for r in range(args.rounds + 1):                      # round 0: untimed
                    dt_a, loss_a, acc_a = run(cfg, mdl, evl, loss_fn, loader, os.path.join(tmp, f"a{tag}{r}"), **hip)
                    dt_b, loss_b, acc_b = run(cfg, mdl, evl, loss_fn, loader, os.path.join(tmp, f"b{tag}{r}"), val_graph=True, **hip)
                    assert evl.val_path == "graph"
                    st = dict(evl.val_graph_stats)
                    dt_c = loop_c()
                    dt_d, loss_d, acc_d = run(cfg, mdl, evl_d, loss_fn, loader, os.path.join(tmp, f"d{tag}{r}"), val_graph=True, query_bank=True, **hip)
                    assert evl_d.val_path == "graph"
                    st_d = dict(evl_d.val_graph_stats)
                    ref = ref or (loss_a, acc_a)
                    equal = equal and (loss_b, acc_b) == ref and (loss_a, acc_a) == ref and (loss_d, acc_d) == ref
                    if r == 0:
                        continue
                    rates["existing"].append(nq / dt_a)
                    rates["val_graph"].append(nq / dt_b)
                    rates["ceiling"].append(len(full) * B / dt_c)
                    rates["query_bank"].append(nq / dt_d)
                    host_us.append(st["host_s"] / st["steps"] * 1e6)
                    host_us_d.append(st_d["host_s"] / st_d["steps"] * 1e6)
                s = {k: summary(v) for k, v in rates.items()}
                s["val_graph_host_us_per_batch"] = statistics.median(host_us)
                s["query_bank_host_us_per_batch"] = statistics.median(host_us_d)
                s["host_us_per_batch_rounds"] = {"val_graph": host_us, "query_bank": host_us_d}
                s["staging_bytes_per_query"] = {"val_graph": st["staging_bytes"] / B, "query_bank": st_d["staging_bytes"] / B}
                s["query_bank_bytes"] = st_d["query_bank_bytes"]
                s["query_bank_over_val_graph"] = s["query_bank"]["queries_per_s_median"] / s["val_graph"]["queries_per_s_median"]
                s["query_bank_range_wholly_above_val_graph"] = s["query_bank"]["queries_per_s_min"] > s["val_graph"]["queries_per_s_max"]
                s["query_bank_fraction_of_ceiling"] = s["query_bank"]["queries_per_s_median"] / s["ceiling"]["queries_per_s_median"]
                s["val_graph_over_existing"] = s["val_graph"]["queries_per_s_median"] / s["existing"]["queries_per_s_median"]
                s["val_graph_range_wholly_above_existing"] = s["val_graph"]["queries_per_s_min"] > s["existing"]["queries_per_s_max"]
                s["val_graph_fraction_of_ceiling"] = s["val_graph"]["queries_per_s_median"] / s["ceiling"]["queries_per_s_median"]
                s["val_loss"], s["val_acc"] = ref
                s["all_loops_return_the_same_loss_and_metrics"] = equal
                res["settings"][tag] = s
                print(key, tag, json.dumps({k: round(v["queries_per_s_median"]) for k, v in s.items() if isinstance(v, dict) and "rounds" in v}),
                      "host us/batch (b)", round(s["val_graph_host_us_per_batch"], 1), "(d)", round(s["query_bank_host_us_per_batch"], 1),
                      "(d) above (b):", s["query_bank_range_wholly_above_val_graph"], "equal:", equal, flush=True)
            bank.check()
            allres[key] = res
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            json.dump(allres, open(OUT, "w"), indent=1)
            del pipe_c, evl, evl_d, mdl, bank
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
