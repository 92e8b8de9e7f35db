"""ms per training step with frozen stages, timed alternately in one process (median of `--rounds` rounds of `--steps` steps, with
the spread), in fp32 and amp bf16:

  cfg 2 (full/cfg2_vog_spat_gt5_bs4):   (a) the full step; (b) freeze = enc, lang from the raw batch; (c) the same from cached rows -
      encoder outputs and argument vectors as EncodedBank / LangBank hold them (the engine's own vog_ctx_encode_videos and
      vog_lang_forward, resident in HBM), so the step starts at vog_concat_rows_f32 / vog_conc_f32_fwd
  cfg 5 (full/cfg5_vog_svsq_gt5_bs16):  (a) the full step; (d) freeze = enc, obj, lang from obj_tx rows and argument vectors as
      ObjBank / LangBank hold them
  the optimiser call alone over the cfg-2 parameter set: vog_opt_step_f32 against vog_opt_step_groups_f32 with 1 and 3 groups
  `--parent DIR`: a checkout of the parent commit (built); its full step is timed in the same rounds under the name `parent_full`

    python scratch/time_finetune.py OUT.json [--rounds N] [--steps K] [--parent DIR]
"""
import ctypes as C
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from tests.gpu_util import comm_for, encoded, objed  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
L = importlib.import_module("vognet-pytorch_amd.lib")
E = importlib.import_module("vognet-pytorch_amd.engine")
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")

CFG2, CFG5 = "full/cfg2_vog_spat_gt5_bs4", "full/cfg5_vog_svsq_gt5_bs16"


def load_parent(path):
    """The parent commit's package under another name (its own libvog_hip.so next to it)."""
    pkg = os.path.join(path, "vognet-pytorch_amd")
    spec = importlib.util.spec_from_file_location("vog_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vog_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("vog_parent.train"), importlib.import_module("vog_parent.mdl_selector")


def setup(name, freeze):
    cfg, sd, batch, c = cases.build(name)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    # the rows the banks would hold for this batch, from the engine's 16-bit inference kernels
    eng = E.VogEngine(cfg, comm_for(c))
    eng.load_state_dict(sd)
    T = int(batch["srl_arg_word_mask_len"].max())
    B = dev["num_cmp_msk"].shape[0]
    lang, fh = eng.encode_queries({k: dev[k] for k in E.LANG_KEYS}, B, T)
    rows = objed(eng, dev) if "obj" in freeze else encoded(eng, dev)
    cached = {k: v for k, v in rows.items() if k not in E.WORD_KEYS}
    cached["lang_arg_vec"] = lang.clone()
    if eng.sep:
        cached["lang_final_hidden"] = fh.clone()
    cached = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in cached.items()}
    torch.cuda.synchronize()
    del eng
    return cfg, sd, c, sel, dev, cached


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "spread": float(np.max(v) - np.min(v)), "all": v}


def step_variants(name, freeze, rounds, steps, parent):
    cfg, sd, c, sel, dev, cached = setup(name, freeze)
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    loss_fn = sel["loss"](cfg, comm_for(c))
    fns = {}
    for tag, amp in (("fp32", None), ("amp_bf16", "bf16")):
        full = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp)
        raw = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, freeze=freeze)
        fed = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, freeze=freeze)
        fns[f"{tag}/full"] = lambda t=full: t.step(dev)
        fns[f"{tag}/frozen_raw"] = lambda t=raw: t.step(dev)
        fns[f"{tag}/frozen_cached"] = lambda t=fed: t.step(cached)
        if parent is not None:
            ptrn, psel = parent
            ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))
            pt = ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp)
            fns[f"{tag}/parent_full"] = lambda t=pt: t.step(dev)
    # before anything is timed: the cached rows give the raw-fed frozen forward (16-bit kernels against the fp32 prefix)
    probe = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, freeze=freeze)
    a, b = probe.forward(cached)[0]["mdl_outs"], probe.forward(dev)[0]["mdl_outs"]
    dev_rel = float((a - b).abs().max() / b.abs().max())
    loss_cached = float(probe.gradients(cached)[0]["loss"])
    assert np.isfinite(loss_cached) and dev_rel <= 1e-3, (dev_rel, loss_cached)
    del probe
    res = {m: [] for m in fns}
    for _ in range(rounds):                                       # the variants alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    out = {m: stats(v) for m, v in res.items()}
    for tag in ("fp32", "amp_bf16"):
        a = out[f"{tag}/full"]["median"]
        for v in ("frozen_raw", "frozen_cached"):
            out[f"{tag}/{v}"]["gain_over_full_ms"] = a - out[f"{tag}/{v}"]["median"]
        if parent is not None:
            p = out[f"{tag}/parent_full"]
            out[f"{tag}/full"]["minus_parent_median_ms"] = a - p["median"]
            out[f"{tag}/full"]["no_regression"] = bool(a - p["median"] <= p["spread"])
    losses = {m: float(fn()["loss"]) for m, fn in fns.items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    return {"case": name, "freeze": list(freeze), "cached_vs_raw_mdl_outs_rel_to_largest": dev_rel, "loss_after": losses,
            "variants_ms": out}, (cfg, sdt, c, loss_fn)


def optimizer_only(ctx, calls=200):
    cfg, sdt, c, loss_fn = ctx
    tr = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4)
    lib = tr.lib
    keys = sorted(k for k, v in tr.params.items())
    gen = torch.Generator(device="cuda").manual_seed(0)
    P = [tr.params[k].clone() for k in keys]
    G = [(torch.rand(p.shape, device="cuda", generator=gen) + 1e-3) * 1e-2 for p in P]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    total = sum(p.numel() for p in P)
    arr = (L.OptTensor * len(P))()
    for i in range(len(P)):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = L.ptr(P[i]), L.ptr(G[i]), L.ptr(M[i]), L.ptr(V[i]), P[i].numel()
    n = len(P)
    cuts = {"groups_1": [(0, n, 1e-4, 0.0)], "groups_3": [(0, n // 3, 1e-4, 0.0), (n // 3, n // 3, 1e-5, 0.01), (2 * (n // 3), n - 2 * (n // 3), 3e-4, 0.0)]}
    count = [0]

    def base(a):
        a.tensors, a.n_tensors = arr, n
        a.lr, a.beta1, a.beta2, a.eps = 1e-4, 0.9, 0.99, 1e-8
        count[0] += 1
        a.step = count[0]

    def plain():
        a = L.OptArgs()
        base(a)
        L.check(lib.vog_opt_step_f32(C.byref(a), L.stream_ptr()), "vog_opt_step_f32")

    def grouped(spans):
        ga = L.OptGroupsArgs()
        base(ga.base)
        garr = (L.OptGroup * len(spans))()
        for i, (f, cnt, lr, wd) in enumerate(spans):
            garr[i].first, garr[i].count, garr[i].lr, garr[i].weight_decay = f, cnt, lr, wd
        ga.groups, ga.n_groups = garr, len(spans)
        L.check(lib.vog_opt_step_groups_f32(C.byref(ga), L.stream_ptr()), "vog_opt_step_groups_f32")

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

    fns = {"vog_opt_step_f32": plain, **{k: (lambda s=s: grouped(s)) for k, s in cuts.items()}}
    res = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            res[k].append(event_ms(fn))
    return {"tensors": n, "elements": total, "calls_per_measurement": calls, "mode": "A",
            "ms_per_call": {k: stats(v) for k, v in res.items()}}


def main():
    torch.cuda.set_device(0)
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    cfg2, ctx = step_variants(CFG2, ("enc", "lang"), rounds, steps, parent)
    opt = optimizer_only(ctx)
    del ctx
    torch.cuda.empty_cache()
    cfg5, _ = step_variants(CFG5, ("enc", "obj", "lang"), rounds, steps, parent)
    summary = {"rounds": rounds, "steps_per_round": steps, "device": torch.cuda.get_device_name(0), "parent_timed": parent is not None,
               "cfg2": cfg2, "cfg5": cfg5, "optimizer_only_cfg2": opt}
    print(json.dumps({k: {m: round(v["median"], 3) for m, v in summary[k]["variants_ms"].items()} for k in ("cfg2", "cfg5")}))
    print(json.dumps({k: round(v["median"], 4) for k, v in opt["ms_per_call"].items()}))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
