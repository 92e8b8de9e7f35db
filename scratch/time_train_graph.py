"""The captured training step (`FP32Trainer.capture`, one graph launch per iteration) against the eager step, timed alternately in
one process at cfg 2 and cfg 5, in fp32 and in amp bf16, each with the defaults and with the fastest recorded opt-ins:

  parent   the parent commit's eager step (`--parent DIR`: a built checkout of it);
  eager    this tree's eager step;
  graph    `slot.step(batch)`, wall time per iteration with the device drained at the end of a round;
  host     the host time until `slot.step` returns (no device wait), per iteration;

median of `--rounds` rounds of `--steps` steps with max - min. Before anything is timed the fp32 default parameters after three
steps of parent and this tree are compared bit for bit (`Drop` gained a field). `nodes`: the captured graph's node count
(`slot.nodes()`). The record is written first; then the script asserts on it that the parameters were bit-equal and that this
tree's eager default lies inside the parent's spread (max - min of the parent's rounds) in every arm.

    python scratch/time_train_graph.py OUT.json [--rounds N] [--steps K] [--parent DIR]
"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import cases  # noqa: E402
from tests.gpu_util import comm_for  # noqa: E402
from time_avg import bit_equal_after_three_steps  # noqa: E402
from time_finetune import load_parent, stats, timed  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
CASES = {"cfg2": "full/cfg2_vog_spat_gt5_bs4", "cfg5": "full/cfg5_vog_svsq_gt5_bs16"}
OPT_INS = {None: dict(attn="fused_pipe", lstm="fused", qkv="factored"),
           "bf16": dict(attn="fused_pipe", lstm_amp="split", gemm_amp="pipe", qkv="factored")}


def host_ms(fn, steps):
    """ms per call until the call returns; the device is drained before and after, outside the clock."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    dt = (time.perf_counter() - t0) / steps * 1e3
    torch.cuda.synchronize()
    return dt


def step(case, rounds, steps, parent):
    cfg, sd, batch, c = cases.build(case)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    loss_fn = sel["loss"](cfg, comm_for(c))
    W = int(dev["srl_arg_word_mask"].shape[-1])

    def mk(amp, **kw):
        return trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, **kw)

    summary = {"case": case, "rounds": rounds, "steps_per_round": steps, "parent_timed": parent is not None, "T": W,
               "longest": int(dev["srl_arg_word_mask_len"].max())}
    fns, hosts, slots = {}, {}, {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp, **kw):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp, **kw)
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = bit_equal_after_three_steps(mk_parent, mk, dev)
    for tag, amp in (("fp32", None), ("amp_bf16", "bf16")):
        for form, kw in (("default", {}), ("opt_ins", OPT_INS[amp])):
            arm = f"{tag}/{form}"
            if parent is not None:
                fns[f"{arm}/parent"] = lambda t=mk_parent(amp, **kw): t.step(dev)
            fns[f"{arm}/eager"] = lambda t=mk(amp, **kw): t.step(dev)
            tr = mk(amp, **kw)
            slot = tr.capture(dev, T=W, keep_graph=True)
            slots[arm] = slot
            fns[f"{arm}/graph"] = lambda s=slot: s.step(dev)
            hosts[f"{arm}/host"] = lambda s=slot: s.step(dev)
    res = {m: [] for m in list(fns) + list(hosts)}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
        for m, fn in hosts.items():
            res[m].append(host_ms(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    for arm, slot in slots.items():
        slot.check()
        e, g = arms[f"{arm}/eager"], arms[f"{arm}/graph"]
        g["minus_eager_median_ms"] = g["median"] - e["median"]
        g["faster_beyond_spread"] = bool(e["median"] - g["median"] > max(e["spread"], g["spread"]))
        g["nodes"] = slot.nodes()
        g["last_loss"] = float(slot.losses(1)[0]["loss"])
        if parent is not None:
            p = arms[f"{arm}/parent"]
            e["minus_parent_median_ms"] = e["median"] - p["median"]
            e["within_parent_spread"] = bool(abs(e["median"] - p["median"]) <= p["spread"])
    summary["arms_ms"] = arms
    print(case, json.dumps({m: [round(v["median"], 3), round(v["spread"], 3)] for m, v in arms.items()}), flush=True)
    return summary


def main():
    torch.cuda.set_device(0)
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    summary = {"device": torch.cuda.get_device_name(0)}
    for tag, case in CASES.items():
        summary[f"{tag}_step"] = step(case, rounds, steps, parent)
        torch.cuda.empty_cache()
    if parent is not None:
        for tag in CASES:
            s = summary[f"{tag}_step"]
            summary[f"{tag}_eager_default_within_parent_spread"] = {
                t: s["arms_ms"][f"{t}/default/eager"]["within_parent_spread"] for t in ("fp32", "amp_bf16")}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)
    if parent is not None:                                          # the assertions on the record
        for tag in CASES:
            assert summary[f"{tag}_step"]["fp32_params_bit_equal_to_parent_after_3_steps"], tag
            assert all(summary[f"{tag}_eager_default_within_parent_spread"].values()), (tag, summary[f"{tag}_eager_default_within_parent_spread"])


if __name__ == "__main__":
    main()
