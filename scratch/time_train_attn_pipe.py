"""The pipelined kernels of the fused training attention (`attn="fused_pipe"`: fa_*_pipe_kernel, csrc/train_attn.hip) against the
plain fused kernels (`attn="fused"`) and the materialised operator (`vog_attn_f32`), timed alternately in one process:

  (a) the operator alone, forward + backward from the kept forward, event-timed, fp32 and amp bf16, at obj_tx / mul_tx of cfg 2
      and at 100 proposals per frame: median of `--rounds` rounds with max - min, the scratch bytes of each form, and what has
      to hold - fused_pipe faster than fused at 100 proposals per frame by more than the larger spread, not slower beyond the
      spread at cfg 2;
  (b) the cfg-2 training step (full/cfg2_vog_spat_gt5_bs4), median of `--rounds` rounds of `--steps` steps with the spread:
      the parent commit's package (`--parent DIR`: a built checkout of it), this tree with the default, attn="fused" and
      attn="fused_pipe", in fp32 and in amp bf16 - and, before anything is timed, the fp32 parameters after 3 steps of parent
      and default, and of "fused" and "fused_pipe", compared bit for bit.

    python scratch/time_train_attn_pipe.py OUT.json [--rounds N] [--steps K] [--parent DIR] [--skip-p100]
"""
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import cases  # noqa: E402
from tests.gpu_util import comm_for  # noqa: E402
from time_avg import bit_equal_after_three_steps  # noqa: E402
from time_finetune import load_parent, stats, timed  # noqa: E402
from time_train_attn import CFG2, SHAPES  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
BW = importlib.import_module("vognet-pytorch_amd.backward")
L = importlib.import_module("vognet-pytorch_amd.lib")
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
FORMS = ("materialized", "fused", "fused_pipe")


def operator_alone(skip_p100, rounds):
    lib = L.load()
    out = {}
    for name, S, N, n, d, H, calls in SHAPES:
        if skip_p100 and "p100" in name:
            continue
        g = torch.Generator().manual_seed(S * 1000 + N)
        x = torch.randn(S * N, d, generator=g).cuda()
        w = {k: (torch.randn(d, d, generator=g) / math.sqrt(d)).cuda() for k in ("wq", "wk", "wv")}
        props = (torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])).cuda()
        pe = (torch.randn(H, 5, generator=g).cuda(), (torch.randn(H, generator=g) * 0.3).cuda())
        boxes = BW._Boxes(props, 720.0, 405.0, 10.0)
        d_cat = torch.randn(S * N, d, generator=g).cuda()
        nf = int(lib.vog_attn_fused_scratch_bytes(S, N, n, d, H))
        nb = {"materialized": int(lib.vog_attn_f32_scratch_bytes(S, N, n, d)), "fused": nf, "fused_pipe": nf}
        scr = {"materialized": torch.empty(nb["materialized"], dtype=torch.uint8, device="cuda"),
               "fused": torch.empty(nf, dtype=torch.uint8, device="cuda")}
        scr["fused_pipe"] = scr["fused"]

        def fwd_bwd(form):
            fused = form != "materialized"
            L.check(lib.vog_train_set_int(b"attn_fused_pipe", int(form == "fused_pipe")), "attn_fused_pipe")
            try:
                f = BW._attn_call(w, pe, x, S, N, n, H, boxes, scratch=scr[form], fused=fused)
                kept = dict(lse=f["lse"], cat=f["cat"]) if fused else {}
                return BW._attn_call(w, pe, x, S, N, n, H, boxes, d_cat=d_cat, scratch=scr[form], fused=fused, **kept)
            finally:
                lib.vog_train_set_int(b"attn_fused_pipe", 0)

        row = {"S": S, "N": N, "n": n, "d": d, "heads": H, "scratch_bytes": nb, "calls_per_timing": calls}
        for tag, amp in (("fp32", 0), ("amp_bf16", 1)):
            L.check(lib.vog_train_set_int(b"amp", amp), "amp")
            try:
                ms = {form: [] for form in FORMS}
                got = {form: fwd_bwd(form) for form in FORMS}
                torch.cuda.synchronize()
                same = all(torch.equal(got["fused"][k], got["fused_pipe"][k]) for k in got["fused"] if torch.is_tensor(got["fused"][k]))
                del got
                for _ in range(rounds):                             # the forms alternate
                    for form in ms:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(calls):
                            fwd_bwd(form)
                        e1.record()
                        torch.cuda.synchronize()
                        ms[form].append(e0.elapsed_time(e1) / calls)
            finally:
                lib.vog_train_set_int(b"amp", 0)
            r = {form: stats(v) for form, v in ms.items()}
            spread = max(r["fused"]["spread"], r["fused_pipe"]["spread"])
            r["pipe_bits_equal_fused"] = bool(same)
            r["fused_over_materialized"] = r["fused"]["median"] / r["materialized"]["median"]
            r["fused_pipe_over_materialized"] = r["fused_pipe"]["median"] / r["materialized"]["median"]
            r["fused_pipe_over_fused"] = r["fused_pipe"]["median"] / r["fused"]["median"]
            r["fused_minus_fused_pipe_ms"] = r["fused"]["median"] - r["fused_pipe"]["median"]
            r["larger_spread_ms"] = spread
            if "p100" in name:
                r["holds"] = bool(r["fused_minus_fused_pipe_ms"] > spread)            # faster by more than the larger spread
            else:
                r["holds"] = bool(-r["fused_minus_fused_pipe_ms"] <= spread)          # not slower beyond the spread
            row[tag] = r
        out[name] = row
        print(name, json.dumps({t: {f: round(row[t][f]["median"], 3) for f in FORMS} for t in ("fp32", "amp_bf16")}),
              {t: (row[t]["holds"], row[t]["pipe_bits_equal_fused"]) for t in ("fp32", "amp_bf16")}, flush=True)
        del scr
        torch.cuda.empty_cache()
    return out


def cfg2_step(rounds, steps, parent):
    cfg, sd, batch, c = cases.build(CFG2)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    loss_fn = sel["loss"](cfg, comm_for(c))

    def mk(amp, **kw):
        return trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, **kw)

    summary = {"case": CFG2, "rounds": rounds, "steps_per_round": steps, "parent_timed": parent is not None}
    summary["fp32_params_fused_pipe_bit_equal_to_fused_after_3_steps"] = bit_equal_after_three_steps(
        lambda amp: mk(amp, attn="fused"), lambda amp: mk(amp, attn="fused_pipe"), dev)
    fns = {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp)
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = bit_equal_after_three_steps(mk_parent, mk, dev)
        fns["fp32/parent"] = lambda t=mk_parent(None): t.step(dev)
        fns["amp_bf16/parent"] = lambda t=mk_parent("bf16"): t.step(dev)
    for tag, amp in (("fp32", None), ("amp_bf16", "bf16")):
        fns[f"{tag}/default"] = lambda t=mk(amp): t.step(dev)
        fns[f"{tag}/fused"] = lambda t=mk(amp, attn="fused"): t.step(dev)
        fns[f"{tag}/fused_pipe"] = lambda t=mk(amp, attn="fused_pipe"): t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    for tag in ("fp32", "amp_bf16"):
        if parent is not None:
            p, dflt = arms[f"{tag}/parent"], arms[f"{tag}/default"]
            dflt["minus_parent_median_ms"] = dflt["median"] - p["median"]
            dflt["within_parent_spread"] = bool(abs(dflt["median"] - p["median"]) <= p["spread"])
        for form in ("fused", "fused_pipe"):
            arms[f"{tag}/{form}"]["minus_default_median_ms"] = arms[f"{tag}/{form}"]["median"] - arms[f"{tag}/default"]["median"]
    summary["arms_ms"] = arms
    losses = {m: float(fn()["loss"]) for m, fn in fns.items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    summary["loss_after"] = losses
    print(json.dumps({m: round(v["median"], 3) for m, v in arms.items()}), flush=True)
    return summary


def main():
    torch.cuda.set_device(0)
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    summary = {"device": torch.cuda.get_device_name(0)}
    summary["operator_alone_ms"] = operator_alone("--skip-p100" in sys.argv, max(rounds, 3))
    summary["cfg2_step"] = cfg2_step(rounds, steps, parent)
    summary["cfg4_step"] = "not run"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
