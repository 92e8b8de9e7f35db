"""ms per training step with weight averaging, timed alternately in one process (median of `--rounds` rounds of `--steps` steps,
with the spread), cfg 2 (full/cfg2_vog_spat_gt5_bs4) in fp32 and amp bf16:

  (a) parent    the parent commit's step (`--parent DIR`: a built checkout of it, e.g. a `git worktree`)
  (b) off       this tree, averaging off (the default)
  (c) ema       FP32Trainer(avg="ema"): vog_opt_average_f32 behind every step
  (d) ema_every4  the same with avg_every=4 (three of four calls return from the decision's w = 0)
  (e) foreach_lerp  the plain step followed by torch._foreach_lerp_ over the same tensors: the unfused host-driven alternative

and, before anything is timed, the fp32 parameters after 3 steps of (a) and (b) compared bit for bit. The averaging call alone
(event-timed over the cfg-2 parameter set) is reported beside the traffic it moves: 3 x 4 bytes per parameter.

    python scratch/time_avg.py OUT.json [--rounds N] [--steps K] [--parent DIR]
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import cases  # noqa: E402
from tests.gpu_util import comm_for  # noqa: E402
from time_finetune import load_parent, stats, timed  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")

CFG2 = "full/cfg2_vog_spat_gt5_bs4"


def bit_equal_after_three_steps(mk_parent, mk_off, dev):
    a, b = mk_parent(None), mk_off(None)
    for _ in range(3):
        a.step(dev)
        b.step(dev)
    torch.cuda.synchronize()
    return bool(all(torch.equal(a.params[k], b.params[k]) for k in b.params) and set(a.params) == set(b.params))


def averaging_call_alone(tr, dev, calls=200):
    """ms per vog_opt_average_f32 over the trainer's own tensors (event-timed), first with w != 0, then skipped (start far away)."""
    tr.step(dev)
    keys = sorted(tr.avg)
    out = {}
    for tag, start in (("applied", 1), ("skipped", 1 << 30)):
        tr.avg_start = start
        for _ in range(20):
            tr._average(keys)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            tr._average(keys)
        e1.record()
        torch.cuda.synchronize()
        out[tag] = e0.elapsed_time(e1) / calls
    elems = sum(tr.avg[k].numel() for k in keys)
    out.update(tensors=len(keys), elements=elems, bytes_moved=12 * elems, gb_per_s_applied=12 * elems / out["applied"] / 1e6)
    return out


def main():
    torch.cuda.set_device(0)
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    cfg, sd, batch, c = cases.build(CFG2)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    loss_fn = sel["loss"](cfg, comm_for(c))

    def mk(amp, **kw):
        return trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, **kw)

    summary = {"case": CFG2, "rounds": rounds, "steps_per_round": steps, "device": torch.cuda.get_device_name(0),
               "parent_timed": parent is not None}
    mk_parent = None
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp)
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = bit_equal_after_three_steps(mk_parent, mk, dev)
    fns = {}
    for tag, amp in (("fp32", None), ("amp_bf16", "bf16")):
        if mk_parent is not None:
            fns[f"{tag}/parent"] = lambda t=mk_parent(amp): t.step(dev)
        fns[f"{tag}/off"] = lambda t=mk(amp): t.step(dev)
        fns[f"{tag}/ema"] = lambda t=mk(amp, avg="ema"): t.step(dev)
        fns[f"{tag}/ema_every4"] = lambda t=mk(amp, avg="ema", avg_every=4): t.step(dev)
        host = mk(amp)
        host.step(dev)                                              # (m / v exist: the tensors the step covers)
        hk = sorted(host.m)
        havg, hp = [torch.zeros_like(host.params[k]) for k in hk], [host.params[k] for k in hk]

        def lerp_step(t=host, a=havg, p=hp):
            r = t.step(dev)
            torch._foreach_lerp_(a, p, 1.0 - 0.999)
            return r
        fns[f"{tag}/foreach_lerp"] = lerp_step
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    for tag in ("fp32", "amp_bf16"):
        off = arms[f"{tag}/off"]["median"]
        for v in ("ema", "ema_every4", "foreach_lerp"):
            arms[f"{tag}/{v}"]["minus_off_median_ms"] = arms[f"{tag}/{v}"]["median"] - off
        if parent is not None:
            p = arms[f"{tag}/parent"]
            arms[f"{tag}/off"]["minus_parent_median_ms"] = off - p["median"]
            arms[f"{tag}/off"]["within_parent_spread"] = bool(abs(off - p["median"]) <= p["spread"])
    summary["arms_ms"] = arms
    losses = {m: float(fn()["loss"]) for m, fn in fns.items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    summary["loss_after"] = losses
    summary["averaging_call_alone_ms"] = averaging_call_alone(mk(None, avg="ema"), dev)
    print(json.dumps({m: round(v["median"], 3) for m, v in arms.items()}))
    print(json.dumps({k: v for k, v in summary.items() if k not in ("arms_ms", "loss_after")}))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
