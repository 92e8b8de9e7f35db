"""What an object-transformer bank buys the fed forward-only loop of sep / svsq models (writes profiles/obj_bank.json; bench.py
is untouched).

    python scratch/time_obj_bank.py [--workload cfg5|sep4|svsq_p100] [--queries 20000] [--rounds 5] [--videos 4096]
    python scratch/time_obj_bank.py --parent --tag parent --root <checkout of the parent commit, built>

One process, the loops ALTERNATED round by round (a difference only counts against the spread of a loop's own rounds):
  (a) bank_f16   engine.FedPipeline from an f16 FeatureBank (raw features: gather, both encoders, concat, obj_tx per batch)
  (b) bank_enc   the same from the EncodedBank of the same videos (gather of encoder outputs, vis_concat, obj_tx)
  (c) bank_obj   the same from the ObjBank (gather of obj_tx's output rows, obj_restore; the forward starts at mul_tx)
A step = one batch of the workload; queries/s = B * steps / seconds, host clock around work that ends in a synchronise.
`--parent` runs (a) and (b) with nothing this file's commit added, so that the same file measures the parent commit from a
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
OUT = os.path.join(HERE_ROOT, "profiles", "obj_bank.json")
VOCAB = 5000
STAGED = ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture",
          "srl_arg_inds_msk", "num_cmp_msk", "verb_ind_in_srl")
WORKLOADS = {
    "cfg5": dict(mdl="vog", conc="svsq", exp="gt5", B=16, tx="f16", desc="VOGNet svsq gt5 + pred_cmp bs=16 fp16 (cfg 5)"),
    "sep4": dict(mdl="vog", conc="sep", exp="gt5", B=4, tx="f16", desc="VOGNet sep gt5 bs=4 fp16"),
    "svsq_p100": dict(mdl="vog", conc="svsq", exp="p100", B=16, tx="f16", desc="VOGNet svsq p100 bs=16 fp16"),
}


def gathered_bytes_per_query(ncmp, nfrm0, nppf0, prop_w, seg_w, elem):
    """vog_assemble_from_bank per query, from the shapes: every feature element read once (`elem` bytes) and written once
    (fp32); proposals read and written (28 B a row)."""
    feat = ncmp * nfrm0 * (nppf0 * prop_w + seg_w)
    props = ncmp * nfrm0 * nppf0 * 28
    return {"read": feat * elem + props, "write": feat * 4 + props}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg5", choices=sorted(WORKLOADS))
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--videos", type=int, default=4096)
    ap.add_argument("--parent", action="store_true")
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
    w = WORKLOADS[args.workload]
    cfg = bench.make_cfg(w)
    nppf0 = ec.num_prop_per_frm(cfg)
    comm = {"vocab_size": VOCAB, "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1}, "num_prop_per_frm": nppf0}
    eng = eng_mod.VogEngine(cfg, comm)
    eng.load_state_dict(synth.init_state_dict(cfg, VOCAB, seed=1))
    B, ncmp, ns = w["B"], (1 if w["conc"] == "svsq" else 4), 4
    steps = max(1, args.queries // B)
    pool = [torch.cuda.Stream(device=dev) for _ in range(16)]         # created back to back, before any slot (see bench.py)
    sts = pool[:ns]
    batch = synth.make_batch(w["conc"], B, nppf0, ncmp=ncmp, vocab_size=VOCAB, seed=2000)
    T = int(batch["srl_arg_word_mask_len"].max())

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
    spec = {"vid_index": np.zeros((B, ncmp), np.int32), **{k: np.zeros_like(batch[k]) for k in STAGED}}

    def fed(bk):
        ex = bk(torch.from_numpy(idx_pool[0]).cuda(), with_loss_keys=False)
        ex.pop("_keepalive")
        ex.update({k: torch.from_numpy(batch[k]) for k in STAGED})
        pipe = eng_mod.FedPipeline(eng, ex, spec, bk, streams=ns, slots_per_stream=2, T=T, stream_pool=sts)
        for st in pipe.stagings:
            st.fill({k: batch[k] for k in STAGED})

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

    banks = {"bank_f16": bank, "bank_enc": dls.EncodedBank.encode(bank, eng, B, ncmp)}
    if not args.parent:
        banks["bank_obj"] = dls.ObjBank.encode(bank, eng, B, ncmp)
    pipes, loops = {}, {}
    for k, bk in banks.items():
        pipes[k], loops[k] = fed(bk)
    for _ in range(3):                         # clocks up, every shape warm
        for step in loops.values():
            timed(step, args.warmup)
    rates = {k: [] for k in loops}
    for _ in range(args.rounds):
        for k, step in loops.items():
            timed(step, 16)
            rates[k].append(B * steps / timed(step, steps))
    for bk in banks.values():
        bk.check()
    # the fed loops computed the same thing: the last batch of every pipeline, same indices
    for sb, sc in zip(pipes["bank_f16"].slots, pipes["bank_enc"].slots):
        assert torch.equal(sb.out["mdl_outs"], sc.out["mdl_outs"]), "encoded and raw fed slots disagree"
    for p in pipes.values():
        for sl in p.slots:
            assert torch.isfinite(sl.out["mdl_outs"]).all()

    def summary(v):
        med = statistics.median(v)
        return {"queries_per_s_median": med, "queries_per_s_min": min(v), "queries_per_s_max": max(v),
                "spread": (max(v) - min(v)) / med, "us_per_step_median": B / med * 1e6, "rounds": v}

    res = {"loops_" + args.tag: {k: summary(v) for k, v in rates.items()}}
    d = eng.desc
    if not args.parent:
        obj, enc = banks["bank_obj"], banks["bank_enc"]
        dev_out = max(float((sb.out["mdl_outs"] - sc.out["mdl_outs"]).abs().max()) for sb, sc in zip(pipes["bank_f16"].slots, pipes["bank_obj"].slots))
        rows = B * ncmp * d.nfrm0 * nppf0
        if obj.lossless_for(eng):
            assert dev_out == 0.0, "cached and raw fed slots disagree inside one tail band"
        res.update({
            "workload": w["desc"], "queries_per_round": B * steps, "rounds": args.rounds, "plan": eng.plan, "streams": ns,
            "bank_videos": args.videos, "rows_per_batch": rows, "tail_band_rows": eng.obj_band_rows(),
            "obj_bit_equal_to_raw": obj.lossless_for(eng), "obj_vs_raw_max_abs_mdl_outs": dev_out,
            "bytes_per_video": {"f16": dls.FeatureBank.bytes_per_video(nppf0, bank.prop_dim, bank.seg_dim, bank.G, "f16"),
                                "enc": dls.EncodedBank.bytes_per_video(nppf0, d.prop_enc, d.seg_enc, enc.G),
                                "obj": dls.ObjBank.bytes_per_video(nppf0, d.prop_enc, d.seg_enc, obj.G)},
            "gathered_bytes_per_query": {"f16": gathered_bytes_per_query(ncmp, d.nfrm0, nppf0, d.prop_dim, d.seg_dim, 2),
                                         "enc": gathered_bytes_per_query(ncmp, d.nfrm0, nppf0, d.prop_enc, d.seg_enc, 4),
                                         "obj": gathered_bytes_per_query(ncmp, d.nfrm0, nppf0, d.prop_enc + d.seg_enc, d.seg_enc, 4)},
            "encode_seconds": {"enc": enc.encode_seconds, "obj": obj.encode_seconds},
            "encode_videos_per_s": {"enc": args.videos / enc.encode_seconds, "obj": args.videos / obj.encode_seconds},
            "observed_logit_max_after_encode": list(eng.observed_logit_max()),
            **{"trace_" + k[5:]: eng.describe_steps(p.slots[0].batch, p.slots[0].ws) for k, p in pipes.items()}})
        lo = res["loops_" + args.tag]
        for other in ("enc", "f16"):
            res["obj_over_" + other] = lo["bank_obj"]["queries_per_s_median"] / lo["bank_" + other]["queries_per_s_median"]
            res["obj_exceeds_%s_by_more_than_its_spread" % other] = lo["bank_obj"]["queries_per_s_min"] > lo["bank_" + other]["queries_per_s_max"]
    allres = json.load(open(OUT)) if os.path.isfile(OUT) else {}
    allres.setdefault(args.workload, {}).update(res)
    cur = allres[args.workload]
    if "loops_parent" in cur and "loops_this" in cur:
        p, t = cur["loops_parent"]["bank_enc"], cur["loops_this"]["bank_enc"]
        margin = p["queries_per_s_max"] - p["queries_per_s_min"]
        cur["enc_this_within_parent_spread_of_parent_median"] = abs(t["queries_per_s_median"] - p["queries_per_s_median"]) <= margin
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(allres, open(OUT, "w"), indent=1)
    print(args.workload, args.tag, json.dumps({k: {"median": round(v["queries_per_s_median"]), "min": round(v["queries_per_s_min"]),
                                                   "max": round(v["queries_per_s_max"])} for k, v in res["loops_" + args.tag].items()}))
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("loops_") and not k.startswith("trace")}))


if __name__ == "__main__":
    main()
