"""What it costs to bring changed parameters into a finalized inference engine (writes profiles/weight_refresh.json; bench.py
is untouched).

    python scratch/time_weight_refresh.py [--rounds 5] [--cases cfg2,cfg4] [--no-learner]

One process. Per case (full-size cfg 2 spat gt5, cfg 4 spat p100; B = 4) the parameters sit on the device in fp32, as
`FP32Trainer.params` do, and change between rounds (a small in-place update), and two paths are ALTERNATED round by round after
one untimed round of each (other people's work shares the host: a difference only counts against the spread of a path's own
rounds):
  (a) host    what `Learner._sync_model` does with cfg.hip.weight_refresh = host: clone the parameters (`state_dict`),
              `mdl.load_state_dict`, `mdl.refresh_weights()` (through the CPU, vog_ctx_finalize), then the slot every captured
              consumer needs again: `make_slot(graph=True)` and its first launch
  (b) device  `mdl.refresh_from_device(params)` (vog_ctx_refresh_device: the pack kernels of csrc/wpack.hip, in place), then a
              launch of the slot that was captured before the first round
Seconds are a host clock around work that ends in a device synchronise. After every round the two engines' outputs on the same
batch are compared for equal bytes (a path that is faster and different is not faster).

The Learner's turn-around (cfg 2 only): two Learners with cfg.hip.val_graph, one per mode, take the same training step; timed
is `Learner.validate` on the smallest loader the annotations allow (one full-shape batch through the validation graph and one
batch a query short), from behind the step's synchronise to behind the validation's - the sync of the model, the bank
checks, the (re)built or reused pipeline, the fed launch, the log read back, the metrics. Alternated the same way.

"faster" is claimed only if EVERY round of (b) is below EVERY round of (a): `device_below_host_in_every_round`.
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
OUT = os.path.join(ROOT, "profiles", "weight_refresh.json")
CASES = {"cfg2": "full/cfg2_vog_spat_gt5_bs4", "cfg4": "full/cfg4_vog_spat_p100_bs4"}
OUT_KEYS = ("mdl_outs", "mdl_outs_eval", "pred_rec")


def summary(v):
    med = statistics.median(v)
    return {"ms_median": med * 1e3, "ms_min": min(v) * 1e3, "ms_max": max(v) * 1e3, "spread": (max(v) - min(v)) / med,
            "rounds_ms": [x * 1e3 for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="cfg2,cfg4")
    ap.add_argument("--no-learner", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from oracle import cases
    T = importlib.import_module("tests.test_gpu_device_metrics")
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: there is no fallback, and a CPU run says nothing about these times")
    torch.cuda.set_device(0)
    res = {"rounds": args.rounds, "cases": {}}

    for key in [c for c in args.cases.split(",") if c]:
        cfg, sd, batch, c = cases.build(CASES[key])
        comm = {"vocab_size": c["vocab"], "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1}, "num_prop_per_frm": c["nppf0"]}
        sel = sel_mod.get_mdl_loss_eval(cfg)
        dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        Tm = int(batch["srl_arg_word_mask_len"].max())
        params = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sd.items()}
        gen = torch.Generator(device="cuda").manual_seed(5)
        mdls = {}
        for mode in ("host", "device"):
            m = sel["mdl"](cfg=cfg, comm=comm)
            m.load_state_dict({k: v.cpu() for k, v in params.items()})
            m.engine()
            mdls[mode] = m
        slot_dev = mdls["device"].engine().make_slot(dev, T=Tm, graph=True)
        slot_dev.launch()
        torch.cuda.synchronize()

        def path_host():
            m = mdls["host"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.load_state_dict({k: v.clone() for k, v in params.items()}, strict=False)
            eng = m.refresh_weights()
            slot = eng.make_slot(dev, T=Tm, graph=True)
            out = slot.launch()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, {k: out[k].clone() for k in OUT_KEYS}

        def path_device():
            m = mdls["device"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            how = m.refresh_from_device(params)
            out = slot_dev.launch()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert how == "in_place", how
            return dt, {k: out[k].clone() for k in OUT_KEYS}

        times = {"host": [], "device": []}
        equal = True
        for r in range(args.rounds + 1):                       # (round 0 is not timed)
            for v in params.values():                          # the parameters move, as after an optimiser step
                v.add_(torch.randn(v.shape, device="cuda", generator=gen) * 1e-4)
            order = (path_host, path_device) if r % 2 == 0 else (path_device, path_host)
            got = {}
            for fn in order:
                dt, out = fn()
                got[fn.__name__] = out
                if r > 0:
                    times["host" if fn is path_host else "device"].append(dt)
            equal = equal and all(torch.equal(got["path_host"][k], got["path_device"][k]) for k in OUT_KEYS)
        one = {"host": summary(times["host"]), "device": summary(times["device"]), "outputs_byte_equal_every_round": bool(equal),
               "device_below_host_in_every_round": max(times["device"]) < min(times["host"]),
               "weights": int(sum(v.numel() for v in params.values())),
               "images": len(mdls["device"].engine().weight_images()),
               "image_bytes": int(sum(r["bytes"] for r in mdls["device"].engine().weight_images())),
               "plan": mdls["device"].engine().plan}
        print(key, json.dumps(one))
        res["cases"][key] = one
        del mdls, slot_dev, params
        torch.cuda.empty_cache()

    if not args.no_learner:
        name = CASES["cfg2"]
        with tempfile.TemporaryDirectory() as tmp:
            learners = {}
            for mode in ("host", "device"):
                cfg, sd, comm, sel, dl = T.make_eval_set(name, os.path.join(tmp, "ann_" + mode), n_batches=2, B=4)
                cfg.hip.val_graph, cfg.hip.device_metrics, cfg.hip.val_pickle, cfg.hip.weight_refresh = True, True, False, mode
                torch.manual_seed(11)
                mdl, evl, loss_fn = T._evaluator(cfg, sd, comm, sel)
                data = tu.DataWrap(path=os.path.join(tmp, mode), train_dl=dl[:1], valid_dl=dl)
                learners[mode] = (tu.Learner(uid="W", data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm), dl, evl)
            times = {"host": [], "device": []}
            vals = {"host": [], "device": []}
            for r in range(args.rounds + 1):
                for mode in (("host", "device") if r % 2 == 0 else ("device", "host")):
                    learn, dl, evl = learners[mode]
                    learn.trainer.step({k: v.to(learn.trainer.dev) for k, v in dl[0].items()})
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    vl, va, _ = learn.validate({"valid": dl})
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    assert evl.val_path == "graph"
                    vals[mode].append({k: float(v) for k, v in vl.items()})
                    if r > 0:
                        times[mode].append(dt)
            res["learner_turnaround_cfg2"] = {
                "host": summary(times["host"]), "device": summary(times["device"]),
                "validation_loss_equal_every_round": vals["host"] == vals["device"],
                "device_below_host_in_every_round": max(times["device"]) < min(times["host"])}
            print("learner", json.dumps(res["learner_turnaround_cfg2"]))

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
