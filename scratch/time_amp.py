"""ms per cfg-2 training step in the four precision modes of the training path, timed alternately in one process:
FP32Trainer.step and the autograd step (loss.backward() + torch.optim.Adam) in fp32, bf16_gemm, amp bf16 and amp f16
(autograd: torch.autocast; f16 with torch.amp.GradScaler; the autograd path has no bf16_gemm mode).

    python scratch/time_amp.py OUT.json [--rounds N] [--steps K]
    python scratch/time_amp.py --profile K        # K amp-bf16 FP32Trainer steps only (for rocprofv3 --kernel-trace --stats)
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
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")

NAME = "full/cfg2_vog_spat_gt5_bs4"


def setup():
    cfg, sd, batch, c = cases.build(NAME)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    return cfg, sd, c, sel, dev


def main():
    torch.cuda.set_device(0)
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
