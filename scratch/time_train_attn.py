"""The fused training attention (`vog_attn_fused_f32`, csrc/train_attn.hip) against the materialised one (`vog_attn_f32`), timed
alternately in one process:

  (a) the operator alone, forward + backward, event-timed, fp32 and amp bf16, at obj_tx / mul_tx of cfg 2 and at 100 proposals
      per frame, with the scratch bytes of both forms;
  (b) the cfg-2 training step (full/cfg2_vog_spat_gt5_bs4), median of `--rounds` rounds of `--steps` steps with the spread:
      the parent commit's package (`--parent DIR`: a built checkout of it), this tree with the default, attn="fused" in fp32 and
      in amp bf16 - and, before anything is timed, the fp32 parameters after 3 steps of parent and default compared bit for bit.

    python scratch/time_train_attn.py OUT.json [--rounds N] [--steps K] [--parent DIR] [--skip-p100]
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

trn = importlib.import_module("vognet-pytorch_amd.train")
BW = importlib.import_module("vognet-pytorch_amd.backward")
L = importlib.import_module("vognet-pytorch_amd.lib")
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")

CFG2 = "full/cfg2_vog_spat_gt5_bs4"
# (name, S, N, n, d, H, calls per timing)
SHAPES = [("obj_tx cfg2", 4, 200, 200, 512, 3, 20), ("mul_tx cfg2", 40, 100, 20, 768, 3, 20),
          ("mul_tx p100", 40, 2000, 400, 768, 3, 2), ("obj_tx p100", 4, 4000, 4000, 512, 3, 2)]


def operator_alone(skip_p100):
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
        nb = {"materialized": int(lib.vog_attn_f32_scratch_bytes(S, N, n, d)), "fused": int(lib.vog_attn_fused_scratch_bytes(S, N, n, d, H))}
        scr = {k: torch.empty(v, dtype=torch.uint8, device="cuda") for k, v in nb.items()}

        def fwd_bwd(form):
            fused = form == "fused"
            f = BW._attn_call(w, pe, x, S, N, n, H, boxes, scratch=scr[form], fused=fused)
            kept = dict(lse=f["lse"], cat=f["cat"]) if fused else {}
            return BW._attn_call(w, pe, x, S, N, n, H, boxes, d_cat=d_cat, scratch=scr[form], fused=fused, **kept)

        row = {"S": S, "N": N, "n": n, "d": d, "heads": H, "scratch_bytes": nb, "calls_per_timing": calls}
        for tag, amp in (("fp32", 0), ("amp_bf16", 1)):
            L.check(lib.vog_train_set_int(b"amp", amp), "amp")
            try:
                ms = {"materialized": [], "fused": []}
                for form in ms:
                    fwd_bwd(form)
                torch.cuda.synchronize()
                for _ in range(3):                                  # the forms alternate
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
            row[tag] = {form: stats(v) for form, v in ms.items()}
            row[tag]["fused_over_materialized"] = row[tag]["fused"]["median"] / row[tag]["materialized"]["median"]
        out[name] = row
        print(name, json.dumps({t: {f: round(row[t][f]["median"], 3) for f in ("materialized", "fused")} for t in ("fp32", "amp_bf16")}),
              flush=True)
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
    fns = {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp)
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = bit_equal_after_three_steps(mk_parent, mk, dev)
        fns["fp32/parent"] = lambda t=mk_parent(None): t.step(dev)
    fns["fp32/default"] = lambda t=mk(None): t.step(dev)
    fns["fp32/fused"] = lambda t=mk(None, attn="fused"): t.step(dev)
    fns["amp_bf16/default"] = lambda t=mk("bf16"): t.step(dev)
    fns["amp_bf16/fused"] = lambda t=mk("bf16", attn="fused"): t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    if parent is not None:
        p, dflt = arms["fp32/parent"], arms["fp32/default"]
        dflt["minus_parent_median_ms"] = dflt["median"] - p["median"]
        dflt["within_parent_spread"] = bool(abs(dflt["median"] - p["median"]) <= p["spread"])
    for tag in ("fp32", "amp_bf16"):
        arms[f"{tag}/fused"]["minus_default_median_ms"] = arms[f"{tag}/fused"]["median"] - arms[f"{tag}/default"]["median"]
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
    summary["operator_alone_ms"] = operator_alone("--skip-p100" in sys.argv)
    summary["cfg2_step"] = cfg2_step(rounds, steps, parent)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
