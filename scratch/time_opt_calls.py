"""The optimiser's calls alone, one build of the library against another (opt_onebody: one apply and one statistics kernel against
the parent's two of each), and the cfg-2 fp32 training step beside them.

    python scratch/time_opt_calls.py PARENT_LIB.so OUT.json [--runs N]    # PARENT_LIB: libvog_hip.so built from the parent commit
    python scratch/time_opt_calls.py --child                              # (one fresh process per run, library from VOG_HIP_LIB)

The parent process starts `--runs` (3) children per library, alternating parent, new, parent, new, ... Each child takes the
cfg-2 parameter set (full/cfg2_vog_spat_gt5_bs4: the tensors its trainer steps, 57 of them, 46.8 M elements) and times with
device events over 200 calls, median of three measurements: vog_opt_step_f32 in mode A and in mode B with max_norm = 1,
vog_opt_step_ex_f32 as AdamW (weight decay 0.01) and as AMSGrad, vog_opt_accum_f32 and vog_opt_average_f32 (EMA, applied);
then FP32Trainer.step, median of five rounds of ten steps (host clock around a device synchronise).

A figure PASSES when the new library's median over its runs is no higher than the parent's median plus the parent's own
max - min over its runs: the margin is the parent's measured noise."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAME = "full/cfg2_vog_spat_gt5_bs4"
CALLS = 200


def child():
    import numpy as np
    import torch
    from oracle import cases
    from tests.gpu_util import comm_for
    trn = importlib.import_module("vognet-pytorch_amd.train")
    L = importlib.import_module("vognet-pytorch_amd.lib")
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    torch.cuda.set_device(0)
    cfg, sd, batch, c = cases.build(NAME)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    loss_fn = sel_mod.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))
    tr = trn.FP32Trainer(cfg, comm_for(c), {k: torch.from_numpy(v) for k, v in sd.items()}, loss_fn, lr=1e-4)
    tr.step(dev)
    lib, keys = tr.lib, sorted(tr.m)
    gen = torch.Generator(device="cuda").manual_seed(0)
    P = [tr.params[k].clone() for k in keys]
    G = [(torch.rand(p.shape, device="cuda", generator=gen) + 1e-3) * 1e-2 for p in P]
    M, V, X, A = ([torch.zeros_like(p) for p in P] for _ in range(4))
    total = sum(p.numel() for p in P)
    arr = (L.OptTensor * len(P))()
    acc_arr = (L.OptAccumTensor * len(P))()
    avg_arr = (L.OptAvgTensor * len(P))()
    for i in range(len(P)):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = L.ptr(P[i]), L.ptr(G[i]), L.ptr(M[i]), L.ptr(V[i]), P[i].numel()
        acc_arr[i].acc, acc_arr[i].g, acc_arr[i].n = L.ptr(A[i]), L.ptr(G[i]), P[i].numel()
        avg_arr[i].avg, avg_arr[i].p, avg_arr[i].n = L.ptr(A[i]), L.ptr(P[i]), P[i].numel()
    state = torch.frombuffer(bytearray(bytes(L.OptState(scale=1.0))), dtype=torch.int32).cuda()
    avg_state = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch = torch.empty(int(lib.vog_opt_scratch_bytes(len(P), total)), dtype=torch.uint8, device="cuda")
    vm = (C.c_void_p * len(P))(*[L.ptr(x) for x in X])
    garr = (L.OptGroup * 1)()
    garr[0].first, garr[0].count, garr[0].lr, garr[0].weight_decay = 0, len(P), 1e-4, 0.01
    count = [0]

    def base(a, mode_b):
        count[0] += 1
        a.tensors, a.n_tensors = arr, len(P)
        a.lr, a.beta1, a.beta2, a.eps, a.step = 1e-4, 0.9, 0.99, 1e-8, count[0]
        if mode_b:
            a.state, a.scratch, a.scratch_bytes, a.max_norm = L.ptr(state), L.ptr(scratch), scratch.numel(), 1.0
            a.growth_factor, a.backoff_factor, a.growth_interval = 2.0, 0.5, 2000

    def call_step(mode_b):
        a = L.OptArgs()
        base(a, mode_b)
        L.check(lib.vog_opt_step_f32(C.byref(a), L.stream_ptr()), "vog_opt_step_f32")

    def call_ex(flags):
        ex = L.OptExArgs()
        base(ex.groups.base, False)
        ex.groups.groups, ex.groups.n_groups = garr, 1
        ex.flags, ex.grad_scale, ex.vmax = flags, 1.0, vm
        L.check(lib.vog_opt_step_ex_f32(C.byref(ex), L.stream_ptr()), "vog_opt_step_ex_f32")

    def call_accum():
        L.check(lib.vog_opt_accum_f32(acc_arr, len(P), L.stream_ptr()), "vog_opt_accum_f32")

    def call_average():
        count[0] += 1
        a = L.OptAvgArgs()
        a.tensors, a.n_tensors, a.mode, a.decay, a.warmup, a.start, a.every = avg_arr, len(P), 1, 0.999, 0, 1, 1
        a.step, a.state = count[0], L.ptr(avg_state)
        L.check(lib.vog_opt_average_f32(C.byref(a), L.stream_ptr()), "vog_opt_average_f32")

    def event_ms(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / CALLS

    out = {"lib": L.LIB_PATH, "device": torch.cuda.get_device_name(0), "tensors": len(P), "elements": total}
    for name, fn in (("mode_a", lambda: call_step(False)), ("mode_b_max_norm_1", lambda: call_step(True)),
                     ("adamw", lambda: call_ex(L.OPT_DECOUPLED)), ("amsgrad", lambda: call_ex(L.OPT_AMSGRAD)),
                     ("accum", call_accum), ("average_ema", call_average)):
        ms = [event_ms(fn) for _ in range(3)]
        out[name] = {"ms_per_call": float(np.median(ms)), "all_ms": ms}
    out["mode_b_steps_skipped"] = L.OptState.from_buffer_copy(state.cpu().numpy().tobytes()).skipped
    rounds = []
    for _ in range(5):
        tr.step(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            tr.step(dev)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / 10 * 1e3)
    out["train_step_fp32"] = {"ms_per_call": float(np.median(rounds)), "all_ms": rounds}
    print("TIMES " + json.dumps(out))


FIGURES = ("mode_a", "mode_b_max_norm_1", "adamw", "amsgrad", "accum", "average_ema", "train_step_fp32")


def main():
    if "--child" in sys.argv:
        return child()
    parent_lib, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
    got = {"parent": [], "new": []}
    for _ in range(runs):
        for tag, env in (("parent", {"VOG_HIP_LIB": parent_lib}), ("new", {})):
            e = {k: v for k, v in os.environ.items() if k != "VOG_HIP_LIB"}
            e.update(env)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=e, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:])
                raise SystemExit(f"{tag} child ended with {r.returncode}")
            rec = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("TIMES ")][-1][6:])
            assert (rec["lib"] == parent_lib) == (tag == "parent"), rec["lib"]
            got[tag].append(rec)
            print(tag, {k: round(rec[k]["ms_per_call"], 4) for k in FIGURES}, flush=True)
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    report = {"case": NAME, "device": got["new"][0]["device"], "tensors": got["new"][0]["tensors"], "elements": got["new"][0]["elements"],
              "calls_per_measurement": CALLS, "runs_per_library": runs, "figures": {}}
    ok = True
    for k in FIGURES:
        p, n = [r[k]["ms_per_call"] for r in got["parent"]], [r[k]["ms_per_call"] for r in got["new"]]
        margin = max(p) - min(p)
        passed = med(n) <= med(p) + margin
        report["figures"][k] = {"parent_ms": p, "new_ms": n, "parent_median_ms": med(p), "new_median_ms": med(n),
                                "parent_spread_ms": margin, "new_spread_ms": max(n) - min(n), "verdict": "pass" if passed else "FAIL"}
        ok = ok and (passed or k == "train_step_fp32")               # the six calls decide; the whole step is reported beside them
    report["all_calls_pass"] = ok
    report["runs"] = got
    print(json.dumps(report["figures"], indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
