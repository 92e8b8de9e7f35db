"""The factored Q / K / V projections of mul_tx's layer 0 (`qkv="factored"`: vog_attn_f32_vl / vog_attn_fused_f32_vl, the
vl_*_kernel launches of csrc/train_tx.hip) against the dense projections, timed alternately in one process:

  (a) the layer-0 operator alone, forward + backward (all gradients, the input's as d_ps / d_lang - the dense arm pays
      `vog_conc_f32_bwd` for them, as the dense step does), event-timed, fp32 and amp bf16 (gemm_amp_pipe on), for the
      materialised and the pipelined fused operator at mul_tx of cfg 2 and for the fused one at 100 proposals per frame:
      median of `--rounds` rounds with max - min;
  (b) the training step at cfg 2 and cfg 5, median of `--rounds` rounds of `--steps` steps with the spread: the parent commit's
      package (`--parent DIR`: a built checkout of it), this tree's default and qkv="factored", in fp32 and in amp bf16 with
      lstm_amp="split", gemm_amp="pipe", attn="fused_pipe" - and, before anything is timed, the fp32 parameters after 3 steps
      of parent and default compared bit for bit.

    python scratch/time_train_qkv.py OUT.json [--rounds N] [--steps K] [--parent DIR] [--skip-p100]
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
CASES = {"cfg2": "full/cfg2_vog_spat_gt5_bs4", "cfg5": "full/cfg5_vog_svsq_gt5_bs16"}
AMP_KW = dict(lstm_amp="split", gemm_amp="pipe", attn="fused_pipe")
# (name, n_q, nc_v, nfrm, n, nsrl, dobj, dlang, H, operators, calls per timing)
SHAPES = [("mul_tx cfg2", 4, 1, 10, 20, 5, 512, 256, 3, ("materialized", "fused_pipe"), 20),
          ("mul_tx p100", 4, 1, 10, 400, 5, 512, 256, 3, ("fused_pipe",), 2)]


def operator_alone(skip_p100, rounds):
    lib, st = L.load(), L.stream_ptr()
    out = {}
    for name, n_q, nc_v, nfrm, n, nsrl, dobj, dlang, H, ops, calls in SHAPES:
        if skip_p100 and "p100" in name:
            continue
        S, N, d = n_q * nc_v * nfrm, nsrl * n, dobj + dlang
        g = torch.Generator().manual_seed(S * 1000 + N)
        ps, lang = torch.randn(S * n, dobj, generator=g).cuda(), torch.randn(n_q * nsrl, dlang, generator=g).cuda()
        msk = torch.ones(n_q * nsrl, dtype=torch.int64).cuda()
        w = {k: (torch.randn(d, d, generator=g) / math.sqrt(d)).cuda() for k in ("wq", "wk", "wv")}
        props = (torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])).cuda()
        pe = (torch.randn(H, 5, generator=g).cuda(), (torch.randn(H, generator=g) * 0.3).cuda())
        boxes = BW._Boxes(props, 720.0, 405.0, 10.0)
        d_cat = torch.randn(S * N, d, generator=g).cuda()
        vl = BW.FactoredInput(ps, lang, msk, n_q, nc_v, nfrm, n, nsrl)
        x = torch.empty(S * N, d, dtype=torch.float32, device="cuda")
        L.check(lib.vog_conc_f32_fwd(L.ptr(ps), L.ptr(lang), L.ptr(msk), L.ptr(x), n_q, nc_v, nfrm, n, nsrl, dobj, dlang, 0, st), "conc")
        nb = {"materialized": int(lib.vog_attn_f32_scratch_bytes(S, N, n, d)), "fused_pipe": int(lib.vog_attn_fused_scratch_bytes(S, N, n, d, H)),
              "vl": int(lib.vog_attn_vl_scratch_bytes(*vl.geometry()))}
        scr = {k: torch.empty(v, dtype=torch.uint8, device="cuda") for k, v in nb.items() if k == "vl" or k in ops}

        def fwd_bwd(op, factored):
            fused = op != "materialized"
            L.check(lib.vog_train_set_int(b"attn_fused_pipe", int(fused)), "attn_fused_pipe")
            kw = dict(scratch=scr[op], **({"fused": True} if fused else {}), **({"vl": vl, "vl_scratch": scr["vl"]} if factored else {}))
            try:
                f = BW._attn_call(w, pe, x, S, N, n, H, boxes, **kw)
                kept = dict(lse=f["lse"], cat=f["cat"]) if fused else {}
                r = BW._attn_call(w, pe, x, S, N, n, H, boxes, d_cat=d_cat, **kw, **kept)
                if not factored:
                    r["d_ps"], r["d_lang"] = BW.conc_backward(r["d_x"], n_q, nc_v, nfrm, n, nsrl, dobj, inds_msk=msk)
                return r
            finally:
                lib.vog_train_set_int(b"attn_fused_pipe", 0)

        row = {"S": S, "N": N, "n": n, "d": d, "dobj": dobj, "heads": H, "scratch_bytes": nb, "calls_per_timing": calls}
        for tag, amp in (("fp32", 0), ("amp_bf16", 1)):
            L.check(lib.vog_train_set_int(b"amp", amp), "amp")
            L.check(lib.vog_train_set_int(b"gemm_amp_pipe", 1 if amp else 0), "gemm_amp_pipe")
            try:
                arms = [(op, f) for op in ops for f in (False, True)]
                ms = {a: [] for a in arms}
                dev_rel = {}
                for op in ops:                                      # before anything is timed: the two forms agree
                    a, b = fwd_bwd(op, False), fwd_bwd(op, True)
                    torch.cuda.synchronize()
                    dev_rel[op] = {k: float((a[k] - b[k]).abs().max() / a[k].abs().max()) for k in ("g_wq", "g_wk", "g_wv", "d_ps", "d_lang")}
                    del a, b
                for _ in range(rounds):                             # the arms alternate
                    for arm in arms:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(calls):
                            fwd_bwd(*arm)
                        e1.record()
                        torch.cuda.synchronize()
                        ms[arm].append(e0.elapsed_time(e1) / calls)
            finally:
                lib.vog_train_set_int(b"amp", 0)
                lib.vog_train_set_int(b"gemm_amp_pipe", 0)
            r = {}
            for op in ops:
                dn, fc = stats(ms[(op, False)]), stats(ms[(op, True)])
                spread = max(dn["spread"], fc["spread"])
                r[op] = {"dense": dn, "factored": fc, "dense_minus_factored_ms": dn["median"] - fc["median"], "larger_spread_ms": spread,
                         "factored_faster_beyond_spread": bool(dn["median"] - fc["median"] > spread),
                         "factored_vs_dense_max_rel": dev_rel[op]}
            row[tag] = r
        out[name] = row
        print(name, json.dumps({t: {op: [round(row[t][op][f]["median"], 3) for f in ("dense", "factored")] for op in ops}
                                for t in ("fp32", "amp_bf16")}), flush=True)
        del scr, x
        torch.cuda.empty_cache()
    return out


def step(case, rounds, steps, parent):
    cfg, sd, batch, c = cases.build(case)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    loss_fn = sel["loss"](cfg, comm_for(c))

    def mk(amp, **kw):
        return trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, **(AMP_KW if amp else {}), **kw)

    summary = {"case": case, "rounds": rounds, "steps_per_round": steps, "parent_timed": parent is not None}
    fns = {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp, **(AMP_KW if amp else {}))
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = bit_equal_after_three_steps(mk_parent, mk, dev)
        fns["fp32/parent"] = lambda t=mk_parent(None): t.step(dev)
        fns["amp_bf16/parent"] = lambda t=mk_parent("bf16"): t.step(dev)
    for tag, amp in (("fp32", None), ("amp_bf16", "bf16")):
        fns[f"{tag}/default"] = lambda t=mk(amp): t.step(dev)
        fns[f"{tag}/factored"] = lambda t=mk(amp, qkv="factored"): t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    for tag in ("fp32", "amp_bf16"):
        dflt, fc = arms[f"{tag}/default"], arms[f"{tag}/factored"]
        if parent is not None:
            p = arms[f"{tag}/parent"]
            dflt["minus_parent_median_ms"] = dflt["median"] - p["median"]
            dflt["within_parent_spread"] = bool(abs(dflt["median"] - p["median"]) <= p["spread"])
        fc["minus_default_median_ms"] = fc["median"] - dflt["median"]
        fc["faster_beyond_spread"] = bool(dflt["median"] - fc["median"] > max(dflt["spread"], fc["spread"]))
    summary["arms_ms"] = arms
    losses = {m: float(fn()["loss"]) for m, fn in fns.items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    summary["loss_after"] = losses
    print(case, json.dumps({m: [round(v["median"], 3), round(v["spread"], 3)] for m, v in arms.items()}), flush=True)
    return summary


def main():
    torch.cuda.set_device(0)
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    summary = {"device": torch.cuda.get_device_name(0)}
    summary["operator_alone_ms"] = operator_alone("--skip-p100" in sys.argv, max(rounds, 3))
    for tag, case in CASES.items():
        summary[f"{tag}_step"] = step(case, rounds, steps, parent)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
