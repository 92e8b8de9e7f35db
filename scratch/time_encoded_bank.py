"""What an encoded feature bank buys the fed forward-only loop (writes profiles/encoded_bank.json; bench.py is untouched).

    python scratch/time_encoded_bank.py [--workload cfg2|cfg4] [--queries 20000] [--rounds 5] [--videos 4096]
    python scratch/time_encoded_bank.py --raw-only --tag parent --root <checkout of the parent commit, built>

One process, the loops ALTERNATED round by round (a difference only counts against the spread of a loop's own rounds):
  (a) resident   the forward's graph slots with inputs resident on the device (bench.py's loop: 4 streams, one slot each)
  (b) bank_f16   engine.FedPipeline from an f16 FeatureBank (raw features: gather, both encoders, concat per batch)
  (c) bank_enc   engine.FedPipeline from the EncodedBank of the same videos (gather of encoder outputs, vis_concat)
  (d) val_graph  cfg 2 only: (b) and (c) with the validation epilogue (device loss + log row, no pickle) behind the forward
A step = one batch of the workload; queries/s = B * steps / seconds, host clock around work that ends in a synchronise.
`--raw-only` runs (a) and (b) with nothing this file's commit added, so that the same file measures the parent commit from a
checkout of it (`--root`); its figures land under loops_<tag>. The bytes gathered per query come from the shapes.
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
OUT = os.path.join(HERE_ROOT, "profiles", "encoded_bank.json")
VOCAB = 5000
LANG_KEYS = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
             "srl_arg_inds_msk", "num_cmp_msk")


def gathered_bytes_per_query(ncmp, nfrm0, nppf0, prop_w, seg_w, elem):
    """vog_assemble_from_bank per query, from the shapes: every feature element read once (`elem` bytes) and written once
    (fp32); proposals read and written (28 B a row)."""
    feat = ncmp * nfrm0 * (nppf0 * prop_w + seg_w)
    props = ncmp * nfrm0 * nppf0 * 28
    return {"read": feat * elem + props, "write": feat * 4 + props}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg4"])
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--videos", type=int, default=4096)
    ap.add_argument("--raw-only", action="store_true")
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
    B, ncmp, ns = w["B"], 4, 4
    steps = max(1, args.queries // B)
    pool = [torch.cuda.Stream(device=dev) for _ in range(16)]         # created back to back, before any slot (see bench.py)
    sts = pool[:ns]
    batches = [synth.make_batch(w["conc"], B, nppf0, vocab_size=VOCAB, seed=2000 + s) for s in range(ns)]
    T = int(max(b["srl_arg_word_mask_len"].max() for b in batches))

    bank = dls.FeatureBank(cfg, comm, args.videos, dtype="f16")
    chunk = min(256 if nppf0 <= 5 else 16, args.videos)
    it = synth.make_items(chunk, 1, nppf0, seed=3)
    one = {k: np.ascontiguousarray(it[k][:, 0]) for k in dls.BANK_KEYS}
    for s0 in range(0, args.videos, chunk):
        n = min(chunk, args.videos - s0)
        bank.put(s0, {k: v[:n] for k, v in one.items()})
    torch.cuda.synchronize()
    assert bank.lossless_for(eng), eng.plan
    rng = np.random.default_rng(0)
    idx_pool = rng.integers(0, args.videos, size=(1024, B, ncmp)).astype(np.int32)
    spec = {"vid_index": np.zeros((B, ncmp), np.int32), **{k: np.zeros_like(batches[0][k]) for k in LANG_KEYS}}

    def fed(bk, example):
        pipe = eng_mod.FedPipeline(eng, example, spec, bk, streams=ns, slots_per_stream=2, T=T, stream_pool=sts)
        for st in pipe.stagings:
            st.fill({k: batches[0][k] for k in LANG_KEYS})

        def step(i):
            st = pipe.next_staging()
            st.host["vid_index"].copy_(torch.from_numpy(idx_pool[i % 1024]))
            pipe.submit()
        return pipe, step

    def timed(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            step(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    ex_raw = {k: torch.from_numpy(v) for k, v in batches[0].items()}
    slots_a = [eng.make_slot({k: torch.from_numpy(v) for k, v in b.items()}, T=T, graph=True) for b in batches]
    loops = {"resident": lambda i: slots_a[i % ns].launch(sts[i % ns])}
    pipe_b, loops["bank_f16"] = fed(bank, ex_raw)
    pipes = [pipe_b]
    enc = None
    if not args.raw_only:
        enc = dls.EncodedBank.encode(bank, eng, B, ncmp)
        ex_enc = enc(torch.from_numpy(idx_pool[0]).cuda(), with_loss_keys=False)
        ex_enc.pop("_keepalive")
        ex_enc.update({k: torch.from_numpy(batches[0][k]) for k in LANG_KEYS})
        pipe_c, loops["bank_enc"] = fed(enc, ex_enc)
        pipes.append(pipe_c)
    for _ in range(3):                         # clocks up, every shape warm
        for step in loops.values():
            timed(step, args.warmup)
    rates = {k: [] for k in loops}
    for _ in range(args.rounds):
        for k, step in loops.items():
            timed(step, 16)
            rates[k].append(B * steps / timed(step, steps))
    bank.check()
    if enc is not None:
        enc.check()
        # the two fed loops computed the same thing: the last batch of either pipeline, same indices
        for sb, sc in zip(pipes[0].slots, pipes[1].slots):
            assert torch.equal(sb.out["mdl_outs"], sc.out["mdl_outs"]), "encoded and raw fed slots disagree"
    for p in pipes:
        for sl in p.slots:
            assert torch.isfinite(sl.out["mdl_outs"]).all()

    def summary(v):
        med = statistics.median(v)
        return {"queries_per_s_median": med, "queries_per_s_min": min(v), "queries_per_s_max": max(v),
                "spread": (max(v) - min(v)) / med, "us_per_step_median": B / med * 1e6, "rounds": v}

    res = {"loops_" + args.tag: {k: summary(v) for k, v in rates.items()}}
    d = eng.desc
    if enc is not None:
        res.update({
            "workload": w["desc"], "queries_per_round": B * steps, "rounds": args.rounds, "plan": eng.plan, "streams": ns,
            "bank_videos": args.videos,
            "bytes_per_video": {"f16": dls.FeatureBank.bytes_per_video(nppf0, bank.prop_dim, bank.seg_dim, bank.G, "f16"),
                                "enc": dls.EncodedBank.bytes_per_video(nppf0, enc.prop_dim, enc.seg_dim, enc.G)},
            "gathered_bytes_per_query": {"f16": gathered_bytes_per_query(ncmp, d.nfrm0, nppf0, d.prop_dim, d.seg_dim, 2),
                                         "enc": gathered_bytes_per_query(ncmp, d.nfrm0, nppf0, d.prop_enc, d.seg_enc, 4)},
            "encode_seconds": enc.encode_seconds, "encode_videos_per_s": args.videos / enc.encode_seconds,
            "trace_raw": eng.describe_steps(pipes[0].slots[0].batch, pipes[0].slots[0].ws),
            "trace_enc": eng.describe_steps(pipes[1].slots[0].batch, pipes[1].slots[0].ws)})
        lo = res["loops_" + args.tag]
        res["enc_over_f16"] = lo["bank_enc"]["queries_per_s_median"] / lo["bank_f16"]["queries_per_s_median"]
        res["enc_exceeds_f16_by_more_than_its_spread"] = lo["bank_enc"]["queries_per_s_min"] > lo["bank_f16"]["queries_per_s_max"]
        if args.workload == "cfg2":
            try:
                res["val_graph"] = val_graph_loop(eng, cfg, comm, bank, enc, batches[0], idx_pool, B, ncmp, T, ns, sts, steps,
                                                  args.rounds, timed, summary)
            except Exception as e:                 # (the forward-only figures above are kept either way)
                res["val_graph"] = {"error": f"{type(e).__name__}: {e}"}
    allres = json.load(open(OUT)) if os.path.isfile(OUT) else {}
    allres.setdefault(args.workload, {}).update(res)
    cur = allres[args.workload]
    if "loops_parent" in cur and "loops_this" in cur:
        p, t = cur["loops_parent"]["bank_f16"], cur["loops_this"]["bank_f16"]
        cur["raw_bank_this_inside_parent_spread"] = p["queries_per_s_min"] <= t["queries_per_s_median"] <= p["queries_per_s_max"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(allres, open(OUT, "w"), indent=1)
    print(json.dumps({k: {"median": round(v["queries_per_s_median"]), "min": round(v["queries_per_s_min"]), "max": round(v["queries_per_s_max"])}
                      for k, v in res["loops_" + args.tag].items()}))
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("loops_") and not k.startswith("trace")}))


def val_graph_loop(eng, cfg, comm, bank, enc, batch, idx_pool, B, ncmp, T, ns, sts, steps, rounds, timed, summary):
    """The same two fed loops with the validation epilogue behind the forward (device loss + the log row; no records kept)."""
    import numpy as np
    import torch
    eng_mod = importlib.import_module("vognet-pytorch_amd.engine")
    dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    sel = importlib.import_module("vognet-pytorch_amd.mdl_selector").get_mdl_loss_eval(cfg)
    loss_fn = sel["loss"](cfg, comm)
    pq = synth.make_items(B, ncmp, 1, prop_dim=4, seg_dim=4, n_gt=bank.G, seed=9)
    rng = np.random.default_rng(1)
    small = {k: batch[k] for k in LANG_KEYS}
    small.update({k: pq[k] for k in dls.PER_QUERY_KEYS})
    small["srl_arg_boxes_mask"] = (batch["srl_arg_inds_msk"] * (rng.uniform(size=batch["srl_arg_inds_msk"].shape) < 0.8)).astype(np.int64)
    rows = 4096
    out = {}
    steps = min(steps, rows)
    for tag, bk in (("bank_f16", bank), ("bank_enc", enc)):
        log = eng_mod.ValLog(eng.device, rows, B, loss=True, words=False, rec_words=0)
        epi = eng_mod.Epilogue(log, loss_fn=loss_fn, grnd_eval=None)
        ex = bk(torch.from_numpy(idx_pool[0]).cuda(), {k: torch.from_numpy(v).cuda() for k, v in pq.items()}, with_loss_keys=False)
        ex.pop("_keepalive")
        ex.update({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in small.items()})
        spec = {"vid_index": np.zeros((B, ncmp), np.int32), **{k: np.zeros_like(v) for k, v in small.items()},
                "val_step": np.zeros(4, np.int32)}
        pipe = eng_mod.FedPipeline(eng, ex, spec, bk, streams=ns, slots_per_stream=2, T=T, stream_pool=sts, epilogue=epi)
        for st in pipe.stagings:
            st.fill(small)

        def step(i, pipe=pipe):
            st = pipe.next_staging()
            st.host["vid_index"].copy_(torch.from_numpy(idx_pool[i % 1024]))
            st.host["val_step"][0] = i % rows
            pipe.submit()
        out[tag] = (pipe, log, step)
    for _ in range(2):
        for _, _, step in out.values():
            timed(step, 40)
    rates = {k: [] for k in out}
    for _ in range(rounds):
        for k, (_, _, step) in out.items():
            rates[k].append(B * steps / timed(step, steps))
    for pipe, log, _ in out.values():
        for sl in pipe.slots:
            sl.check()
        log.check()
    a, b = out["bank_f16"][1].loss[:steps], out["bank_enc"][1].loss[:steps]
    res = {k: summary(v) for k, v in rates.items()}
    res["loss_rows_equal"] = bool(torch.equal(a, b))
    res["queries_per_round"] = B * steps              # (one round fills the validation log once: at most `rows` steps)
    return res


if __name__ == "__main__":
    main()
