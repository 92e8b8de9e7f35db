"""What a language bank buys the fed forward-only loop and the val_graph loop (writes profiles/lang_bank.json; bench.py is
untouched).

    python scratch/time_lang_bank.py [--workload cfg2|cfg5] [--queries 20000] [--rounds 5] [--videos 4096]
    python scratch/time_lang_bank.py --parent-only --tag parent --root <checkout of the parent commit, built>

One process, the loops ALTERNATED round by round (a difference only counts against the spread of a loop's own rounds). Every
loop is an engine.FedPipeline (4 streams x 2 slots) whose staging buffer holds {qry_index, vid_index}:
  (a) qbank         f16 FeatureBank + QueryBank: gather of the word-level rows, the whole forward
  (b) lbank         the same + LangBank: gather of the argument vectors, the forward starts behind the BiLSTM
  (c) banked_p0/p1  EncodedBank (cfg 2) / ObjBank (cfg 5) + LangBank with pair_launches 0 and 1 (1: `bank_prep` where its rule holds)
  (d) --parent-only (a) alone, so that the same file measures the parent commit from a checkout of it (`--root`)
and the same (a) / (b) with the validation epilogue (device loss + log row) behind the forward: the val_graph step.
A step = one batch; queries/s = B * steps / seconds, host clock around work that ends in a synchronise. Also recorded: the
seconds `LangBank.encode` takes for the 20 000 queries at B = 4 and B = 16, and the bank's bytes per query from the shapes.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(HERE_ROOT, "profiles", "lang_bank.json")
VOCAB = 5000
WORD_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture")
SMALL_KEYS = WORD_KEYS + ("srl_arg_inds_msk", "num_cmp_msk", "verb_ind_in_srl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg5"])
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--videos", type=int, default=4096)
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--root", default=HERE_ROOT, help="the checkout whose package and library are measured")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)

    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    ec = importlib.import_module("vognet-pytorch_amd.extended_config")
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    eng_mod = importlib.import_module("vognet-pytorch_amd.engine")
    dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
    assert os.path.abspath(eng_mod.__file__).startswith(root), eng_mod.__file__
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: there is no fallback, and a CPU run says nothing about these rates")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    w = bench.WORKLOADS[args.workload]
    cfg = bench.make_cfg(w)
    nppf0 = ec.num_prop_per_frm(cfg)
    comm = {"vocab_size": VOCAB, "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1}, "num_prop_per_frm": nppf0}
    eng = eng_mod.VogEngine(cfg, comm)
    eng.load_state_dict(synth.init_state_dict(cfg, VOCAB, seed=1))
    sep = w["conc"] in ("sep", "svsq")
    B, ns = w["B"], 4
    steps = max(1, args.queries // B)
    Q = B * steps
    pool = [torch.cuda.Stream(device=dev) for _ in range(16)]         # created back to back, before any slot (see bench.py)
    sts = pool[:ns]

    # the queries: 64 distinct synthetic batches, tiled to Q rows
    distinct = [synth.make_batch(w["conc"], B, nppf0, vocab_size=VOCAB, seed=2000 + s) for s in range(64)]
    ncmp = int(distinct[0]["num_cmp_msk"].shape[1])
    T = int(max(b["srl_arg_word_mask_len"].max() for b in distinct))
    pq = synth.make_items(B, ncmp, 1, prop_dim=4, seg_dim=4, n_gt=4, seed=9)
    rng = np.random.default_rng(1)
    small_keys = [k for k in SMALL_KEYS if k in distinct[0]]

    def small_of(b):
        s = {k: b[k] for k in small_keys}
        s.update({k: pq[k] for k in dls.PER_QUERY_KEYS})
        s["srl_arg_boxes_mask"] = (b["srl_arg_inds_msk"] * (rng.uniform(size=b["srl_arg_inds_msk"].shape) < 0.8)).astype(np.int64)
        if sep:
            s["verb_cmp"] = (rng.uniform(size=(B, ncmp)) < 0.5).astype(np.int64)
            s["verb_cross_cmp_msk"] = (rng.uniform(size=(B, ncmp, ncmp)) < 0.6).astype(np.int64)
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items()}

    smalls = [small_of(b) for b in distinct]
    reps = (steps + len(smalls) - 1) // len(smalls)
    qb = dls.QueryBank.from_batches((smalls * reps)[:steps], host_keys=[])
    assert qb.Q == Q

    bank = dls.FeatureBank(cfg, comm, args.videos, dtype="f16", n_gt=4)
    chunk = min(256, args.videos)
    it = synth.make_items(chunk, 1, nppf0, n_gt=4, seed=3)
    one = {k: np.ascontiguousarray(it[k][:, 0]) for k in dls.BANK_KEYS}
    for s0 in range(0, args.videos, chunk):
        n = min(chunk, args.videos - s0)
        bank.put(s0, {k: v[:n] for k, v in one.items()})
    torch.cuda.synchronize()
    idx_pool = rng.integers(0, args.videos, size=(1024, B, ncmp)).astype(np.int32)
    spec = {"qry_index": np.zeros(B, np.int32), "vid_index": np.zeros((B, ncmp), np.int32)}

    def example(bk, queries):
        ex = bk(torch.from_numpy(idx_pool[0]).cuda(), {k: smalls[0][k].cuda() for k in dls.PER_QUERY_KEYS}, with_loss_keys=False)
        ex.pop("_keepalive")
        rows = queries(torch.arange(B, dtype=torch.int32))
        rows.pop("_keepalive")
        ex.update({k: v for k, v in rows.items() if k not in dls.PER_QUERY_KEYS})
        return ex

    def fed(bk, queries, epilogue=None, rows=0):
        sp = dict(spec)
        if epilogue is not None:
            sp["val_step"] = np.zeros(4, np.int32)
        pipe = eng_mod.FedPipeline(eng, example(bk, queries), sp, bk, streams=ns, slots_per_stream=2, T=T, stream_pool=sts,
                                   epilogue=epilogue, queries=queries)

        def step(i):
            st = pipe.next_staging()
            q0 = (i * B) % Q
            torch.arange(q0, q0 + B, dtype=torch.int32, out=st.host["qry_index"])
            st.host["vid_index"].copy_(torch.from_numpy(idx_pool[i % 1024]))
            if epilogue is not None:
                st.host["val_step"][0] = i % rows
            pipe.submit()
        return pipe, step

    def timed(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            step(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def summary(v):
        med = statistics.median(v)
        return {"queries_per_s_median": med, "queries_per_s_min": min(v), "queries_per_s_max": max(v),
                "spread": (max(v) - min(v)) / med, "us_per_step_median": B / med * 1e6, "rounds": v}

    def run(loops, n_steps, before=None):
        for _ in range(3):                         # clocks up, every shape warm
            for k, step in loops.items():
                if before:
                    before(k)
                timed(step, args.warmup)
        rates = {k: [] for k in loops}
        for _ in range(args.rounds):
            for k, step in loops.items():
                if before:
                    before(k)
                timed(step, 16)
                rates[k].append(B * n_steps / timed(step, n_steps))
        return {k: summary(v) for k, v in rates.items()}

    pipes, loops = {}, {}
    pipes["qbank"], loops["qbank"] = fed(bank, qb)
    res = {}
    lbk = None
    if not args.parent_only:
        enc_seconds = {}
        for Bn in (4, 16):
            lbk = dls.LangBank.encode(qb, eng, Bn, T)
            enc_seconds[f"B{Bn}"] = lbk.encode_seconds
        lbk = dls.LangBank.encode(qb, eng, B, T)                   # the bank the loops read: the workload's own geometry
        pipes["lbank"], loops["lbank"] = fed(bank, lbk)
        vbank = (dls.ObjBank if sep else dls.EncodedBank).encode(bank, eng, B, ncmp)
        eng.set_option("pair_launches", 0)
        pipes["banked_p0"], loops["banked_p0"] = fed(vbank, lbk)
        eng.set_option("pair_launches", 1)
        pipes["banked_p1"], loops["banked_p1"] = fed(vbank, lbk)
        d = eng.desc
        nvl = ncmp if sep else 1
        res.update({
            "workload": w["desc"], "queries": Q, "rounds": args.rounds, "plan": eng.plan, "streams": ns, "T": T,
            "bank_videos": args.videos, "encode_seconds_20000_queries": enc_seconds,
            "bytes_per_query": {"lang_bank_columns": dls.LangBank.bytes_per_query(d.nsrl, d.lang_enc, nvl, sep),
                                "word_level_columns": sum(qb.row_bytes(k) for k in WORD_KEYS),
                                "query_bank": qb.nbytes // Q, "lang_bank": lbk.nbytes // Q},
            "traces": {k: eng.describe_steps(p.slots[0].batch, p.slots[0].ws) for k, p in pipes.items()}})
    res["loops_" + args.tag] = run(loops, steps)
    for k, p in pipes.items():
        for sl in p.slots:
            sl.check()
            assert torch.isfinite(sl.out["mdl_outs"]).all(), k
    if not args.parent_only:
        lo = res["loops_" + args.tag]
        a, b = lo["qbank"], lo["lbank"]
        res["lbank_over_qbank"] = b["queries_per_s_median"] / a["queries_per_s_median"]
        res["lbank_exceeds_qbank_by_more_than_the_spread"] = b["queries_per_s_min"] > a["queries_per_s_max"]
        p0, p1 = lo["banked_p0"], lo["banked_p1"]
        res["bank_prep_over_three_launches"] = p1["queries_per_s_median"] / p0["queries_per_s_median"]
        res["bank_prep_exceeds_three_launches_by_more_than_the_spread"] = p1["queries_per_s_min"] > p0["queries_per_s_max"]
        # the slots of the two banked pipelines ran the same last batches: same bits
        for s0, s1 in zip(pipes["banked_p0"].slots, pipes["banked_p1"].slots):
            assert torch.equal(s0.out["mdl_outs"], s1.out["mdl_outs"]), "bank_prep and the three launches disagree"
        try:
            res["val_graph_" + args.tag] = val_graph_loops(eng, cfg, comm, bank, qb, lbk, fed, run, min(steps, 4096), B)
        except Exception as e:                     # (the forward-only figures above are kept either way)
            res["val_graph_" + args.tag] = {"error": f"{type(e).__name__}: {e}"}
    del pipes
    allres = json.load(open(OUT)) if os.path.isfile(OUT) else {}
    allres.setdefault(args.workload, {}).update(res)
    cur = allres[args.workload]
    if "loops_parent" in cur and "loops_this" in cur:
        p, t = cur["loops_parent"]["qbank"], cur["loops_this"]["qbank"]
        cur["qbank_this_inside_parent_spread"] = p["queries_per_s_min"] <= t["queries_per_s_median"] <= p["queries_per_s_max"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(allres, open(OUT, "w"), indent=1)
    print(json.dumps({k: {"median": round(v["queries_per_s_median"]), "min": round(v["queries_per_s_min"]), "max": round(v["queries_per_s_max"])}
                      for k, v in res["loops_" + args.tag].items()}))
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("loops_") and k != "traces"}))


def val_graph_loops(eng, cfg, comm, bank, qb, lbk, fed, run, rows, B):
    """(a) and (b) with the validation epilogue behind the forward (device loss + the log row; no records kept)."""
    eng_mod = importlib.import_module("vognet-pytorch_amd.engine")
    sel = importlib.import_module("vognet-pytorch_amd.mdl_selector").get_mdl_loss_eval(cfg)
    loss_fn = sel["loss"](cfg, comm)
    loops, keep = {}, []
    for tag, queries in (("qbank", qb), ("lbank", lbk)):
        log = eng_mod.ValLog(eng.device, rows, B, loss=True, words=False, rec_words=0)
        epi = eng_mod.Epilogue(log, loss_fn=loss_fn, grnd_eval=None)
        pipe, loops[tag] = fed(bank, queries, epilogue=epi, rows=rows)
        keep.append((pipe, log))
    res = run(loops, rows)
    for pipe, log in keep:
        for sl in pipe.slots:
            sl.check()
        log.check()
    a, b = res["qbank"], res["lbank"]
    res["lbank_over_qbank"] = b["queries_per_s_median"] / a["queries_per_s_median"]
    res["lbank_exceeds_qbank_by_more_than_the_spread"] = b["queries_per_s_min"] > a["queries_per_s_max"]
    res["loss_rows_max_abs_difference"] = float((keep[0][1].loss[:rows] - keep[1][1].loss[:rows]).abs().max())
    res["steps_per_round"] = rows
    return res


if __name__ == "__main__":
    main()
