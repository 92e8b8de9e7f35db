"""Fused encoder-layer tail at d = 256 / 384 against the unfused chain it replaces, and the default widths against a parent build.

    python scratch/time_tail_widths.py OUT.json [--parent DIR] [--rounds 5]

One process, arms alternated, every shape warmed up first; per figure the median of `--rounds` rounds and max - min.
  (a) operator: vog_time_kernel on the step names of one forward (pair launches off, so that obj_tail is a launch of its own),
      model = vsrl.*_encode_size 128 with every other size at its default, at the cfg-2 geometry (800 obj / 4000 mul rows) and at
      100 proposals per frame (16000 / 80000 rows);
  (b) loop: forward-only graph replay, 4 slots in flight on 4 streams, fused_tail = 1 against 0, same model; and the
      lstm_layer#1 || obj_tail pair launch (pair_mask 15) against the two launches (13);
  (c) --parent DIR (a checkout of the parent commit with its library built): the cfg-2 loop of this tree against the parent's
      package, alternated - the default widths must not move."""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

VOCAB = 5000
UNFUSED = ("wo", "ln1", "ffn1", "ffn2", "ln2")


def load_pkg(root, name):
    if root == ROOT:
        return importlib.import_module("vognet-pytorch_amd")
    d = os.path.join(root, "vognet-pytorch_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def sub(pkg, name):
    return importlib.import_module(pkg.__name__ + "." + name)


def make_engine(pkg, over, tx):
    ec, synth, em = sub(pkg, "extended_config"), sub(pkg, "synth"), sub(pkg, "engine")
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"mdl.name": "vog", "ds.conc_type": "spat", "mdl.obj_tx.use_rel": True, "mdl.mul_tx.use_rel": True, **over})
    cfg.hip.tx_dtype = tx
    nppf0 = ec.num_prop_per_frm(cfg)
    eng = em.VogEngine(cfg, {"vocab_size": VOCAB, "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1}, "num_prop_per_frm": nppf0})
    eng.load_state_dict(synth.init_state_dict(cfg, VOCAB, seed=1))
    batches = [synth.make_batch("spat", 4, nppf0, vocab_size=VOCAB, seed=7 + s) for s in range(4)]
    return eng, batches


def stat(xs):
    return {"median": statistics.median(xs), "spread": max(xs) - min(xs), "rounds": [round(x, 3) for x in xs]}


def operator(eng, batch, rounds, iters=100):
    """us per launch: the fused tails and the sum of the launches they replace"""
    eng.set_option("pair_launches", 0)
    arms = {}
    for ft in (1, 0):
        eng.set_option("fused_tail", ft)
        arms[ft] = eng.make_slot({k: torch.from_numpy(v) for k, v in batch.items()}, graph=False)
        arms[ft].launch()
    torch.cuda.synchronize()
    names = {1: {"obj": ["obj_tail"], "mul": ["mul_tail"]},
             0: {"obj": [f"obj_{s}" for s in UNFUSED], "mul": [f"mul_{s}" for s in UNFUSED] + ["lin2", "score"]}}
    got = {(ft, k): [] for ft in (1, 0) for k in ("obj", "mul")}
    for r in range(rounds + 1):                       # round 0 warms every kernel up
        for ft in (1, 0):
            eng.set_option("fused_tail", ft)
            for k in ("obj", "mul"):
                us = sum(eng.time_kernel(arms[ft], n, iters) for n in names[ft][k])
                if r:
                    got[(ft, k)].append(us)
    eng.set_option("fused_tail", 1)
    eng.set_option("pair_launches", 1)
    return {f"{k}_{'fused' if ft else 'unfused'}_us": stat(v) for (ft, k), v in got.items()}


_STREAMS = []


def loop_arms(arms, rounds, steps=200):
    """arms: {name: [4 captured slots]} -> us per forward, 4 in flight, arms alternated. The four streams are made once per
    process: which hardware queue a new stream lands on moves a loop by tens of percent (seen here: one group of arms at 88 / 134 us
    next to 51 / 81 us for the same forwards), so figures compare within a group of arms and, with shared streams, across groups."""
    if not _STREAMS:
        _STREAMS.extend(torch.cuda.Stream() for _ in range(4))
    streams = _STREAMS

    def run(slots, n):
        for i in range(n):
            slots[i % 4].launch(streams[i % 4])
        torch.cuda.synchronize()

    for slots in arms.values():
        run(slots, 40)
    t_end = time.perf_counter() + 0.03               # clocks up
    while time.perf_counter() < t_end:
        run(next(iter(arms.values())), 40)
    got = {k: [] for k in arms}
    for _ in range(rounds):
        for k, slots in arms.items():
            run(slots, 8)
            t0 = time.perf_counter()
            run(slots, steps)
            got[k].append((time.perf_counter() - t0) / steps * 1e6)
    return {k: stat(v) for k, v in got.items()}


def slots_of(eng, batches):
    return [eng.make_slot({k: torch.from_numpy(v) for k, v in b.items()}, graph=True) for b in batches]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-p100", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    here = load_pkg(ROOT, "here")
    res = {"rounds": a.rounds, "unit": "us", "device": torch.cuda.get_device_name(0)}
    enc128 = {"mdl.vsrl.prop_encode_size": 128, "mdl.vsrl.seg_encode_size": 128, "mdl.vsrl.lang_encode_size": 128}
    for geo, over in (("gt5", {"ds.exp_setting": "gt5"}), ("p100", {"ds.exp_setting": "p100"})):
        if geo == "p100" and a.skip_p100:
            res["p100"] = "not measured"
            continue
        for tx in ("bf16", "f16"):
            eng, batches = make_engine(here, {**enc128, **over}, tx)
            key = f"enc128_{geo}_{tx}"
            res[key] = {"plan": eng.plan, "operator": operator(eng, batches[0], a.rounds)}
            arms = {}
            for ft in (1, 0):
                eng.set_option("fused_tail", ft)
                arms["fused_tail=%d" % ft] = slots_of(eng, batches)
            eng.set_option("fused_tail", 1)
            res[key]["loop_us_per_forward"] = loop_arms(arms, a.rounds)
            # lstm_layer#1 || obj_tail as one launch (pair_mask bit 2) against the two launches
            parm = {}
            for name, mask in (("obj_pair", 15), ("obj_unpaired", 13)):
                eng.set_option("pair_mask", mask)
                parm[name] = slots_of(eng, batches)
            eng.set_option("pair_mask", 15)
            res[key]["pair_loop_us_per_forward"] = loop_arms(parm, a.rounds)
            del parm
            print(key, json.dumps(res[key]), flush=True)
            del arms, eng
    if a.parent:
        par = load_pkg(os.path.abspath(a.parent), "vog_parent")
        e1, b1 = make_engine(here, {}, "bf16")
        e0, b0 = make_engine(par, {}, "bf16")
        res["cfg2_vs_parent"] = {"operator_this_tree": operator(e1, b1[0], a.rounds), "operator_parent": operator(e0, b0[0], a.rounds),
                                 "loop_us_per_forward": loop_arms({"this_tree": slots_of(e1, b1), "parent": slots_of(e0, b0)}, a.rounds)}
        print("cfg2_vs_parent", json.dumps(res["cfg2_vs_parent"]), flush=True)
    else:
        res["cfg2_vs_parent"] = "not measured"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
