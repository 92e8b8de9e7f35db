"""What a device-resident feature bank buys the host-fed loop (writes profiles/feature_bank.json; bench.py is untouched).

    python scratch/time_feature_bank.py [--workload cfg2|cfg4] [--steps 400] [--rounds 5] [--videos 4096]
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/time_feature_bank.py --trace-only      # kernel times, own run
    python scratch/time_feature_bank.py --merge-stats DIR                                             # -> the json's "assembly_kernel"

One process, three loops ALTERNATED round by round (other people's work shares the host; a difference only counts against the
spread of a loop's own rounds):
  (a) resident   the forward's graph slots with inputs resident on the device (bench.py's loop: 4 streams, one slot each)
  (b) host_items engine.FedPipeline from pinned host items - the per-video items cross the host link every step
  (c) bank_f16   engine.FedPipeline from an f16 FeatureBank: the staging buffer holds the video indices and the word arrays;
                 uniformly random indices into a bank far larger than the 256 MiB Infinity Cache: an HBM gather
A step = one batch of the workload; queries/s = B * steps / seconds, host clock around work that ends in a synchronise.
The bytes per query over the link come from `staging.nbytes`; the assembly kernel's bytes come from the shapes (read + write).
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "feature_bank.json")
VOCAB = 5000
LANG_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
             "srl_arg_inds_msk", "num_cmp_msk")


def assembly_bytes(B, ncmp, nfrm0, nppf0, prop_dim, seg_dim, elem):
    """bank_rows_kernel per launch, from the shapes: every gathered element read once (`elem` bytes) and written once (fp32);
    proposals read and written (28 B a row)."""
    feat = B * ncmp * nfrm0 * (nppf0 * prop_dim + seg_dim)
    props = B * ncmp * nfrm0 * nppf0 * 28
    return {"read": feat * elem + props, "write": feat * 4 + props}


def merge_stats(d, key):
    """Kernel rows of a rocprofv3 --kernel-trace --stats run -> profiles/feature_bank.json["assembly_kernel"]."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    hit = [r for r in rows if "bank_rows_kernel" in r.get("Name", "")]
    if not hit:
        raise SystemExit(f"no bank_rows_kernel row under {d}")
    res = json.load(open(OUT))
    r = hit[0]
    ns = float(r["AverageNs"])
    by = res[key]["assembly_bytes_per_launch"]
    gt = [x for x in rows if "bank_gt_kernel" in x.get("Name", "")]
    res[key]["assembly_kernel"] = {
        "name": r["Name"][:80], "calls": int(r["Calls"]), "avg_us": ns / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3,
        "bytes_per_launch": by, "achieved_tb_per_s": (by["read"] + by["write"]) / ns / 1e3,
        "gt_kernel_avg_us": float(gt[0]["AverageNs"]) / 1e3 if gt else None,
        "source": "rocprofv3 --kernel-trace --stats, a run of its own (loop (c) only, 4 forwards in flight beside it)"}
    gap_us = res[key]["loops"]["bank_f16"]["us_per_step_median"] - res[key]["loops"]["resident"]["us_per_step_median"]
    res[key]["assembly_kernel"]["share_of_gap_to_resident"] = (ns / 1e3) / gap_us if gap_us > 0 else None
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res[key]["assembly_kernel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg4"])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--videos", type=int, default=4096)
    ap.add_argument("--trace-only", action="store_true", help="loop (c) alone, for a rocprofv3 run; writes nothing")
    ap.add_argument("--merge-stats", metavar="DIR")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.workload)

    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    ec = importlib.import_module("vognet-pytorch_amd.extended_config")
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    eng_mod = importlib.import_module("vognet-pytorch_amd.engine")
    dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
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
    B, ncmp, ns = w["B"], 4, 4
    pool = [torch.cuda.Stream(device=dev) for _ in range(16)]         # created back to back, before any slot (see bench.py)
    sts = pool[:ns]
    batches = [synth.make_batch(w["conc"], B, nppf0, vocab_size=VOCAB, seed=2000 + s) for s in range(ns)]
    T = int(max(b["srl_arg_word_mask_len"].max() for b in batches))

    # (c) the bank: `videos` segments; 256 distinct synthetic ones repeated (the values do not matter to a gather's time,
    # the addresses do), indices uniformly random
    bank = dls.FeatureBank(cfg, comm, args.videos, dtype="f16")
    chunk = min(256 if nppf0 <= 5 else 16, args.videos)
    it = synth.make_items(chunk, 1, nppf0, seed=3)
    one = {k: np.ascontiguousarray(it[k][:, 0]) for k in dls.BANK_KEYS}
    for s0 in range(0, args.videos, chunk):
        n = min(chunk, args.videos - s0)
        bank.put(s0, {k: v[:n] for k, v in one.items()})
    torch.cuda.synchronize()
    assert bank.lossless_for(eng), eng.plan
    ex = {k: torch.from_numpy(v) for k, v in batches[0].items()}
    spec_c = {"vid_index": np.zeros((B, ncmp), np.int32), **{k: np.zeros_like(batches[0][k]) for k in LANG_KEYS}}
    pipe_c = eng_mod.FedPipeline(eng, ex, spec_c, bank, streams=ns, slots_per_stream=2, T=T, stream_pool=sts)
    rng = np.random.default_rng(0)
    idx_pool = rng.integers(0, args.videos, size=(1024, B, ncmp)).astype(np.int32)
    for st in pipe_c.stagings:
        st.fill({k: batches[0][k] for k in LANG_KEYS})

    def step_c(i):
        st = pipe_c.next_staging()
        st.host["vid_index"].copy_(torch.from_numpy(idx_pool[i % 1024]))
        pipe_c.submit()

    def timed(step, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if args.trace_only:
        timed(step_c, args.warmup)
        dt = timed(step_c, args.steps)
        bank.check()
        print(f"trace run: bank_f16 {B * args.steps / dt:.0f} queries/s (under the tracer: not a result)")
        return

    # (a) resident graph slots
    slots_a = [eng.make_slot({k: torch.from_numpy(v) for k, v in b.items()}, T=T, graph=True) for b in batches]

    def step_a(i):
        slots_a[i % ns].launch(sts[i % ns])

    # (b) FedPipeline from pinned host items: the parent's host-fed path
    asm = dls.DeviceBatchAssembler(cfg, comm)
    items = synth.make_items(B, ncmp, nppf0, seed=5)
    spec_b = {**{k: items[k] for k in dls.FWD_KEYS}, **{k: batches[0][k] for k in LANG_KEYS}}
    pipe_b = eng_mod.FedPipeline(eng, ex, spec_b, asm, streams=ns, slots_per_stream=2, T=T, stream_pool=sts)

    def step_b(i):
        pipe_b.next_staging()                  # (the loader would write the next batch here; its bytes travel either way)
        pipe_b.submit()

    loops = {"resident": step_a, "host_items": step_b, "bank_f16": step_c}
    for _ in range(3):                         # clocks up, every shape warm
        for step in loops.values():
            timed(step, args.warmup)
    rates = {k: [] for k in loops}
    for _ in range(args.rounds):
        for k, step in loops.items():
            timed(step, 16)
            rates[k].append(B * args.steps / timed(step, args.steps))
    bank.check()
    for sl in pipe_b.slots + pipe_c.slots + slots_a:
        assert torch.isfinite(sl.out["mdl_outs"]).all()

    def summary(v):
        med = statistics.median(v)
        return {"queries_per_s_median": med, "queries_per_s_min": min(v), "queries_per_s_max": max(v),
                "spread": (max(v) - min(v)) / med, "us_per_step_median": B / med * 1e6, "rounds": v}

    res = {"loops": {k: summary(v) for k, v in rates.items()}}
    b_, c_, a_ = (res["loops"][k] for k in ("host_items", "bank_f16", "resident"))
    elem = 2
    res.update({
        "workload": w["desc"], "steps": args.steps, "rounds": args.rounds, "plan": eng.plan, "streams": ns, "fed_slots": len(pipe_c.slots),
        "bank": {"videos": args.videos, "dtype": "f16", "nbytes": bank.nbytes,
                 "bytes_per_video": dls.FeatureBank.bytes_per_video(nppf0, bank.prop_dim, bank.seg_dim, bank.G, "f16")},
        "link_bytes_per_query": {"host_items": pipe_b.stagings[0].nbytes / B, "bank_f16": pipe_c.stagings[0].nbytes / B},
        "assembly_bytes_per_launch": assembly_bytes(B, ncmp, bank.nfrm0, nppf0, bank.prop_dim, bank.seg_dim, elem),
        "bank_over_host_items": c_["queries_per_s_median"] / b_["queries_per_s_median"],
        "bank_exceeds_host_items_by_more_than_its_spread": c_["queries_per_s_min"] > b_["queries_per_s_max"],
        "gap_to_resident": 1.0 - c_["queries_per_s_median"] / a_["queries_per_s_median"],
        "gap_to_resident_us_per_step": c_["us_per_step_median"] - a_["us_per_step_median"],
        "assembly_kernel": "not measured (run under rocprofv3, then --merge-stats)"})
    allres = json.load(open(OUT)) if os.path.isfile(OUT) else {}
    allres[args.workload] = res
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(allres, open(OUT, "w"), indent=1)
    print(json.dumps({k: {"median": round(v["queries_per_s_median"]), "spread": round(v["spread"], 4)} for k, v in res["loops"].items()}))
    print(json.dumps({k: res[k] for k in ("link_bytes_per_query", "bank_over_host_items",
                                          "bank_exceeds_host_items_by_more_than_its_spread", "gap_to_resident")}))


if __name__ == "__main__":
    main()
