"""ms per cfg-2 training step in the four precision modes of the training path, timed alternately in one process:
FP32Trainer.step and the autograd step (loss.backward() + torch.optim.Adam) in fp32, bf16_gemm, amp bf16 and amp f16
(autograd: torch.autocast; f16 with torch.amp.GradScaler; the autograd path has no bf16_gemm mode).

    python scratch/time_amp.py OUT.json [--rounds N] [--steps K]
    python scratch/time_amp.py --profile K        # K amp-bf16 FP32Trainer steps only (for rocprofv3 --kernel-trace --stats)
    python scratch/time_amp.py --fused-opt OUT.json [--rounds N] [--steps K]
        # the fused optimiser step (vog_opt_step_f32): four step variants timed alternately - (a) gradients() + the per-tensor
        # vog_adam_f32 loop that FP32Trainer.step ran before the fused call, (b) the default step, (c) step with clip_norm = 1,
        # (d) amp f16 with a dynamic loss scale - and the optimiser call alone over the cfg-2 parameter set with device events,
        # also as vog_opt_step_ex_f32 (AdamW, AMSGrad: 36 bytes per element) and vog_opt_accum_f32
        # (recorded in profiles/train_opt_variants.json)
"""
import contextlib
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from tests.gpu_util import comm_for  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
L = importlib.import_module("vognet-pytorch_amd.lib")
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")

NAME = "full/cfg2_vog_spat_gt5_bs4"


def setup():
    cfg, sd, batch, c = cases.build(NAME)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    return cfg, sd, c, sel, dev


def per_tensor_step(tr, dev):
    """FP32Trainer.step as it was before vog_opt_step_f32: gradients, then one vog_adam_f32 launch per tensor."""
    ld, grads = tr.gradients(dev)
    tr.num_it += 1
    tr.adam_step += 1
    st = L.stream_ptr()
    for k in sorted(grads):
        p = tr.params[k]
        if k not in tr.m:
            tr.m[k], tr.v[k] = torch.zeros_like(p), torch.zeros_like(p)
        gk = grads[k].contiguous()
        L.check(tr.lib.vog_adam_f32(L.ptr(p), L.ptr(gk), L.ptr(tr.m[k]), L.ptr(tr.v[k]), p.numel(), tr.lr, tr.betas[0],
                                    tr.betas[1], tr.eps, tr.adam_step, st), "vog_adam_f32")
    return ld


HBM_ROOF_TBS = 8.0          # MI355X peak HBM bandwidth


def fused_opt(out, rounds, steps, calls=200):
    import ctypes as C
    cfg, sd, c, sel, dev = setup()
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    loss_fn = sel["loss"](cfg, comm_for(c))
    mk = lambda **kw: trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, **kw)
    trainers = {"a_per_tensor_loop": mk(), "b_fused_default": mk(), "c_clip_norm_1": mk(clip_norm=1.0),
                "d_amp_f16_dynamic_scale": mk(amp="f16", loss_scale="dynamic")}
    fns = {m: (lambda t=t: per_tensor_step(t, dev)) if m.startswith("a_") else (lambda t=t: t.step(dev)) for m, t in trainers.items()}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    res = {m: [] for m in fns}
    for _ in range(rounds):                                       # the variants alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn))
    variants = {m: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "all": v} for m, v in res.items()}
    for m in ("c_clip_norm_1", "d_amp_f16_dynamic_scale"):
        variants[m]["scaler_state"] = trainers[m].scaler_state()
    a, b = variants["a_per_tensor_loop"], variants["b_fused_default"]
    cond = {"b_median_minus_a_median_ms": b["median"] - a["median"], "a_range_ms": a["max"] - a["min"],
            "met": bool(b["median"] - a["median"] <= a["max"] - a["min"])}

    # ---- the optimiser call alone: the cfg-2 parameter set, device events
    tr = trainers["b_fused_default"]
    keys = sorted(tr.m)
    lib = tr.lib
    gen = torch.Generator(device="cuda").manual_seed(0)
    P = [tr.params[k].clone() for k in keys]
    G = [(torch.rand(p.shape, device="cuda", generator=gen) + 1e-3) * 1e-2 for p in P]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    total = sum(p.numel() for p in P)
    arr = (L.OptTensor * len(P))()
    for i in range(len(P)):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = L.ptr(P[i]), L.ptr(G[i]), L.ptr(M[i]), L.ptr(V[i]), P[i].numel()
    state = torch.frombuffer(bytearray(bytes(L.OptState(scale=1.0))), dtype=torch.int32).cuda()
    scratch = torch.empty(int(lib.vog_opt_scratch_bytes(len(P), total)), dtype=torch.uint8, device="cuda")
    count = [0]

    def args(mode_b):
        a = L.OptArgs()
        a.tensors, a.n_tensors = arr, len(P)
        a.lr, a.beta1, a.beta2, a.eps = 1e-4, 0.9, 0.99, 1e-8
        if mode_b:
            a.state, a.scratch, a.scratch_bytes, a.max_norm = L.ptr(state), L.ptr(scratch), scratch.numel(), 1.0
            a.growth_factor, a.backoff_factor, a.growth_interval = 2.0, 0.5, 2000
        return a

    def call_loop():
        count[0] += 1
        st = L.stream_ptr()
        for i in range(len(P)):
            L.check(lib.vog_adam_f32(L.ptr(P[i]), L.ptr(G[i]), L.ptr(M[i]), L.ptr(V[i]), P[i].numel(), 1e-4, 0.9, 0.99, 1e-8, count[0], st),
                    "vog_adam_f32")

    def call_fused(mode_b):
        count[0] += 1
        a = args(mode_b)
        a.step = count[0]
        L.check(lib.vog_opt_step_f32(C.byref(a), L.stream_ptr()), "vog_opt_step_f32")

    def event_ms(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    X = [torch.zeros_like(p) for p in P]
    vm = (C.c_void_p * len(P))(*[L.ptr(x) for x in X])
    garr = (L.OptGroup * 1)()
    garr[0].first, garr[0].count, garr[0].lr, garr[0].weight_decay = 0, len(P), 1e-4, 0.01
    acc_arr = (L.OptAccumTensor * len(P))()
    A = [torch.zeros_like(p) for p in P]
    for i in range(len(P)):
        acc_arr[i].acc, acc_arr[i].g, acc_arr[i].n = L.ptr(A[i]), L.ptr(G[i]), P[i].numel()

    def call_ex(flags):
        count[0] += 1
        ex = L.OptExArgs()
        a = ex.groups.base
        a.tensors, a.n_tensors = arr, len(P)
        a.lr, a.beta1, a.beta2, a.eps, a.step = 1e-4, 0.9, 0.99, 1e-8, count[0]
        ex.groups.groups, ex.groups.n_groups = garr, 1
        ex.flags, ex.grad_scale, ex.vmax = flags, 1.0, vm
        L.check(lib.vog_opt_step_ex_f32(C.byref(ex), L.stream_ptr()), "vog_opt_step_ex_f32")

    def call_accum():
        L.check(lib.vog_opt_accum_f32(acc_arr, len(P), L.stream_ptr()), "vog_opt_accum_f32")

    opt = {}
    for name, fn, bpe in (("per_tensor_loop", call_loop, 28), ("fused_mode_a", lambda: call_fused(False), 28),
                          ("fused_mode_b", lambda: call_fused(True), 32), ("ex_adamw_mode_a", lambda: call_ex(L.OPT_DECOUPLED), 28),
                          ("ex_amsgrad_mode_a", lambda: call_ex(L.OPT_AMSGRAD), 36), ("accum", call_accum, 12)):
        ms = [event_ms(fn) for _ in range(3)]
        med = float(np.median(ms))
        tbs = total * bpe / (med * 1e-3) / 1e12
        opt[name] = {"ms_per_call": med, "all_ms": ms, "bytes_per_element": bpe, "bytes_moved": total * bpe, "tb_per_s": tbs,
                     "fraction_of_hbm_roof": tbs / HBM_ROOF_TBS}
    summary = {"case": NAME, "rounds": rounds, "steps_per_round": steps, "device": torch.cuda.get_device_name(0),
               "step_variants_ms": variants, "timing_condition": cond,
               "optimizer_only": {"tensors": len(P), "elements": total, "calls_per_measurement": calls, "hbm_roof_tb_per_s": HBM_ROOF_TBS,
                                  "mode_b_steps_skipped": L.OptState.from_buffer_copy(state.cpu().numpy().tobytes()).skipped, **opt}}
    print(json.dumps({"step_ms": {m: v["median"] for m, v in variants.items()}, "timing_condition": cond,
                      "optimizer_only_ms": {k: v["ms_per_call"] for k, v in opt.items()},
                      "optimizer_only_tb_per_s": {k: v["tb_per_s"] for k, v in opt.items()}}))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


def main():
    torch.cuda.set_device(0)
    if "--fused-opt" in sys.argv:
        out = sys.argv[sys.argv.index("--fused-opt") + 1]
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
        steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
        return fused_opt(out, rounds, steps)
    cfg, sd, c, sel, dev = setup()
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    loss_fn = sel["loss"](cfg, comm_for(c))
    if "--profile" in sys.argv:
        k = int(sys.argv[sys.argv.index("--profile") + 1])
        tr = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp="bf16")
        for _ in range(k):
            tr.step(dev)
        torch.cuda.synchronize()
        return
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    modes = {"fp32": {}, "bf16_gemm": {"bf16_gemm": True}, "amp_bf16": {"amp": "bf16"}, "amp_f16": {"amp": "f16"}}
    trainers = {m: trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, **kw) for m, kw in modes.items()}
    models, opts, scalers = {}, {}, {}
    for m in ("fp32", "amp_bf16", "amp_f16"):
        mdl = sel["mdl"](cfg=cfg, comm=comm_for(c))
        mdl.load_state_dict(sdt)
        mdl = mdl.cuda().eval().requires_grad_(True)
        models[m], opts[m] = mdl, torch.optim.Adam(mdl.parameters(), lr=1e-4, betas=(0.9, 0.99))
        scalers[m] = torch.amp.GradScaler("cuda") if m == "amp_f16" else None
    cast = {"fp32": None, "amp_bf16": torch.bfloat16, "amp_f16": torch.float16}

    def ag_step(m):
        mdl, opt, sc = models[m], opts[m], scalers[m]
        opt.zero_grad()
        ctx = torch.autocast("cuda", dtype=cast[m]) if cast[m] is not None else contextlib.nullcontext()
        with ctx:
            loss = loss_fn(mdl(dev), dev)["loss"]
        if sc is None:
            loss.backward()
            opt.step()
        else:
            sc.scale(loss).backward()
            sc.step(opt)
            sc.update()
        return loss

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    res = {m: {"trainer_step_ms": [], "autograd_step_ms": []} for m in modes}
    for _ in range(rounds):                                       # the modes alternate: drift hits them all alike
        for m in modes:
            res[m]["trainer_step_ms"].append(timed(lambda: trainers[m].step(dev)))
            if m in models:
                res[m]["autograd_step_ms"].append(timed(lambda: ag_step(m)))
    summary = {"case": NAME, "rounds": rounds, "steps_per_round": steps, "device": torch.cuda.get_device_name(0), "modes": {}}
    for m, r in res.items():
        summary["modes"][m] = {k: {"median": float(np.median(v)), "min": float(np.min(v)), "all": v} for k, v in r.items() if v}
        summary["modes"][m]["loss_after"] = float(trainers[m].step(dev)["loss"])
    print(json.dumps({m: {k: v["median"] for k, v in r.items() if isinstance(v, dict)} for m, r in summary["modes"].items()}))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
