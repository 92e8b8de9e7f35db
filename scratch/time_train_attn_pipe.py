"""The two forms of the fused training attention (`attn="fused"`: fa_*_kernel, `attn="fused_pipe"`: fa_*_pipe_kernel,
csrc/train_attn.hip) against each other, against the materialised operator (`vog_attn_f32`) and against the parent commit's
build (`--parent DIR`: a built checkout of it), timed alternately in one process:

  (a) the operator alone. First, with a parent, its bits: forward, stand-alone backward and backward from the kept forward of
      both forms, fp32 and amp bf16, with and without dropout, at BITS_SHAPES - every output `torch.equal` to the parent's. Then
      forward + backward from the kept forward, event-timed, fp32 and amp bf16, at obj_tx / mul_tx of cfg 2 and at 100
      proposals per frame: median of `--rounds` rounds with max - min, the scratch bytes of each form, and what has to hold -
      fused_pipe faster than fused at 100 proposals per frame by more than the larger spread, not slower beyond the spread at
      cfg 2, and each form's median within the larger of the two builds' spreads of the parent's;
  (b) the cfg-2 training step (full/cfg2_vog_spat_gt5_bs4), median of `--rounds` rounds of `--steps` steps with the spread:
      the parent's package and this tree, each with the default, attn="fused" and attn="fused_pipe", in fp32 and in amp bf16 -
      and, before anything is timed, the fp32 parameters after 3 steps compared bit for bit: parent and this tree under the
      default, under "fused" and under "fused_pipe", and "fused" against "fused_pipe".

    python scratch/time_train_attn_pipe.py OUT.json [--rounds N] [--steps K] [--parent DIR] [--skip-p100] [--skip-materialized]
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
# (S, N, n, d, H): head size 16 on both sides of the 16-, 32- and 64-row tiles, and head size 256
BITS_SHAPES = [(2, 17, 17, 48, 3), (2, 65, 65, 48, 3), (2, 129, 129, 48, 3), (2, 100, 20, 768, 3)]
OUTPUTS = ("cat", "lse", "d_x", "g_wq", "g_wk", "g_wv", "g_pe_w", "g_pe_b")


def operands(S, N, n, d, H, bw):
    g = torch.Generator().manual_seed(S * 1000 + N)
    x = torch.randn(S * N, d, generator=g).cuda()
    w = {k: (torch.randn(d, d, generator=g) / math.sqrt(d)).cuda() for k in ("wq", "wk", "wv")}
    props = (torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])).cuda()
    pe = (torch.randn(H, 5, generator=g).cuda(), (torch.randn(H, generator=g) * 0.3).cuda())
    d_cat = torch.randn(S * N, d, generator=g).cuda()
    return x, w, pe, {k: m._Boxes(props, 720.0, 405.0, 10.0) for k, m in bw.items()}, d_cat


def switched(lmod, name, value, fn):
    lib = lmod.load()
    lmod.check(lib.vog_train_set_int(name, value), name.decode())
    try:
        return fn()
    finally:
        lib.vog_train_set_int(name, 0)


def bits_against_parent(pbuild):
    """Every output of the three entries of the operator, this build's against the parent's (each library has its own switches)."""
    builds = {"this": (BW, L), "parent": pbuild}
    out = {}
    for S, N, n, d, H in BITS_SHAPES:
        x, w, pe, boxes, d_cat = operands(S, N, n, d, H, {k: b[0] for k, b in builds.items()})
        for amp in (0, 1):
            for form in ("fused", "fused_pipe"):
                for drop in (None, (0.1, 1234, 3)):
                    got = {}
                    for k, (bw, lmod) in builds.items():
                        def run(bw=bw, k=k):
                            call = lambda **kw: bw._attn_call(w, pe, x, S, N, n, H, boxes[k], drop=drop, fused=True, **kw)
                            f = call()
                            return {"forward": f, "backward": call(d_cat=d_cat), "backward_kept": call(d_cat=d_cat, lse=f["lse"], cat=f["cat"])}
                        got[k] = switched(lmod, b"amp", amp, lambda: switched(lmod, b"attn_fused_pipe", int(form == "fused_pipe"), run))
                    torch.cuda.synchronize()
                    differ = [f"{e}/{o}" for e in got["this"] for o in OUTPUTS
                              if (o in got["this"][e]) != (o in got["parent"][e])
                              or (o in got["this"][e] and not torch.equal(got["this"][e][o], got["parent"][e][o]))]
                    n_cmp = sum(o in got["this"][e] for e in got["this"] for o in OUTPUTS)
                    key = f"S{S} N{N} d{d} H{H} {'bf16' if amp else 'fp32'} {form} {'drop' if drop else 'nodrop'}"
                    out[key] = {"outputs_compared": n_cmp, "differ": differ}
                    print("bits", key, n_cmp, differ or "equal", flush=True)
    return {"cases": out, "all_equal": bool(all(not v["differ"] and v["outputs_compared"] == 14 for v in out.values()))}


def operator_alone(skip_p100, rounds, pbuild, forms):
    lib = L.load()
    builds = {"this": (BW, L)}
    if pbuild is not None:
        builds["parent"] = pbuild
    out = {}
    for name, S, N, n, d, H, calls in SHAPES:
        if skip_p100 and "p100" in name:
            continue
        x, w, pe, boxes, d_cat = operands(S, N, n, d, H, {k: b[0] for k, b in builds.items()})
        nf = int(lib.vog_attn_fused_scratch_bytes(S, N, n, d, H))
        nb = {"materialized": int(lib.vog_attn_f32_scratch_bytes(S, N, n, d)), "fused": nf, "fused_pipe": nf}
        scr = {"fused": torch.empty(nf, dtype=torch.uint8, device="cuda")}
        if "materialized" in forms:
            scr["materialized"] = torch.empty(nb["materialized"], dtype=torch.uint8, device="cuda")
        scr["fused_pipe"] = scr["fused"]
        # the arms: this build's forms, then the parent's two fused forms
        arms = {form: ("this", form) for form in forms}
        if pbuild is not None:
            arms.update({f"parent/{form}": ("parent", form) for form in ("fused", "fused_pipe")})

        def fwd_bwd(arm):
            k, form = arms[arm]
            bw, lmod = builds[k]
            fused = form != "materialized"

            def run():
                f = bw._attn_call(w, pe, x, S, N, n, H, boxes[k], scratch=scr[form], fused=fused)
                kept = dict(lse=f["lse"], cat=f["cat"]) if fused else {}
                return bw._attn_call(w, pe, x, S, N, n, H, boxes[k], d_cat=d_cat, scratch=scr[form], fused=fused, **kept)
            return switched(lmod, b"attn_fused_pipe", int(form == "fused_pipe"), run)

        row = {"S": S, "N": N, "n": n, "d": d, "heads": H, "scratch_bytes": nb, "calls_per_timing": calls}
        for tag, amp in (("fp32", 0), ("amp_bf16", 1)):
            for _, lmod in builds.values():                         # each library has its own amp switch: once per tag
                lmod.check(lmod.load().vog_train_set_int(b"amp", amp), "amp")
            try:
                ms = {arm: [] for arm in arms}
                got = {arm: fwd_bwd(arm) for arm in arms}
                torch.cuda.synchronize()
                eq = lambda p, q: all(torch.equal(got[p][k], got[q][k]) for k in got[p] if torch.is_tensor(got[p][k]))
                same = eq("fused", "fused_pipe")
                same_parent = {form: eq(form, f"parent/{form}") for form in ("fused", "fused_pipe")} if pbuild is not None else None
                del got
                for _ in range(rounds):                             # the arms alternate
                    for arm in ms:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(calls):
                            fwd_bwd(arm)
                        e1.record()
                        torch.cuda.synchronize()
                        ms[arm].append(e0.elapsed_time(e1) / calls)
            finally:
                for _, lmod in builds.values():
                    lmod.load().vog_train_set_int(b"amp", 0)
            r = {arm: stats(v) for arm, v in ms.items()}
            spread = max(r["fused"]["spread"], r["fused_pipe"]["spread"])
            r["pipe_bits_equal_fused"] = bool(same)
            if "materialized" in forms:
                r["fused_over_materialized"] = r["fused"]["median"] / r["materialized"]["median"]
                r["fused_pipe_over_materialized"] = r["fused_pipe"]["median"] / r["materialized"]["median"]
            r["fused_pipe_over_fused"] = r["fused_pipe"]["median"] / r["fused"]["median"]
            r["fused_minus_fused_pipe_ms"] = r["fused"]["median"] - r["fused_pipe"]["median"]
            r["larger_spread_ms"] = spread
            if "p100" in name:
                r["holds"] = bool(r["fused_minus_fused_pipe_ms"] > spread)            # faster by more than the larger spread
            else:
                r["holds"] = bool(-r["fused_minus_fused_pipe_ms"] <= spread)          # not slower beyond the spread
            if pbuild is not None:
                r["bits_equal_parent"] = same_parent
                for form in ("fused", "fused_pipe"):
                    p = r[f"parent/{form}"]
                    r[form]["minus_parent_median_ms"] = r[form]["median"] - p["median"]
                    r[form]["within_larger_spread_of_parent"] = bool(abs(r[form]["median"] - p["median"]) <= max(r[form]["spread"], p["spread"]))
            row[tag] = r
        out[name] = row
        print(name, json.dumps({t: {f: round(row[t][f]["median"], 3) for f in arms} for t in ("fp32", "amp_bf16")}),
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
    arms_of = ("default", "fused", "fused_pipe")
    kw_of = {"default": {}, "fused": {"attn": "fused"}, "fused_pipe": {"attn": "fused_pipe"}}
    fns = {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp, **kw):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp, **kw)
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = {
            arm: bit_equal_after_three_steps(lambda amp: mk_parent(amp, **kw_of[arm]), lambda amp: mk(amp, **kw_of[arm]), dev) for arm in arms_of}
    for tag, amp in (("fp32", None), ("amp_bf16", "bf16")):
        for arm in arms_of:
            if parent is not None:
                fns[f"{tag}/parent/{arm}"] = lambda t=mk_parent(amp, **kw_of[arm]): t.step(dev)
            fns[f"{tag}/{arm}"] = lambda t=mk(amp, **kw_of[arm]): t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    for tag in ("fp32", "amp_bf16"):
        for arm in arms_of:
            if parent is not None:
                p, mine = arms[f"{tag}/parent/{arm}"], arms[f"{tag}/{arm}"]
                mine["minus_parent_median_ms"] = mine["median"] - p["median"]
                mine["within_larger_spread_of_parent"] = bool(abs(mine["median"] - p["median"]) <= max(mine["spread"], p["spread"]))
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
    pbuild = (importlib.import_module("vog_parent.backward"), importlib.import_module("vog_parent.lib")) if parent is not None else None
    forms = tuple(f for f in FORMS if f != "materialized" or "--skip-materialized" not in sys.argv)
    summary = {"device": torch.cuda.get_device_name(0)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1)
    if pbuild is not None:
        summary["operator_bits_against_parent"] = bits_against_parent(pbuild)
        save()
    summary["operator_alone_ms"] = operator_alone("--skip-p100" in sys.argv, max(rounds, 3), pbuild, forms)
    save()
    summary["cfg2_step"] = cfg2_step(rounds, steps, parent)
    summary["cfg4_step"] = "not run"
    save()


if __name__ == "__main__":
    main()
