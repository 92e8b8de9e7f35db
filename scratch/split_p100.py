"""The hi + lo operand plan at 100 proposals per frame (cfg-4 shape, tests/p100_sharp_case.py): envelope series and timing.

    python scratch/split_p100.py model DIR [scale ...]      # CPU: operand-rounding model of the plan (scratch/r6_quant_split.py's
                                                            # scheme) at wq / wk x scale, and the fp32 oracle outputs -> DIR/x<scale>.npz
    python scratch/split_p100.py gpu DIR OUT.json [--rounds N]   # GPU: error of tx_dtype = split against those oracle outputs and the
                                                            # logit maxima the kernels report, per scale; then ms per forward of
                                                            # tx_dtype = split / f32 on the x 16 checkpoint and of auto
                                                            # (f16) on the unsharpened one, alternately in one process
    python scratch/split_p100.py profile K                  # K split forwards only (for rocprofv3 --kernel-trace --stats)
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
from oracle import vog_oracle as vo  # noqa: E402
from tests import p100_sharp_case as pc  # noqa: E402

SCALES = [12.0, 16.0, 20.0, 24.0]


def model(out_dir, scales):
    from scratch.r5_quant_envelope import scheme
    h, SP = torch.float16, "split"
    plans = {"f16": {"tx": h}, "split": {"tx": h, "enc": SP, "enc.lang": h, "tx.proj": SP, "tx.qk": SP}}
    os.makedirs(out_dir, exist_ok=True)
    torch.set_num_threads(16)
    eng = importlib.import_module("vognet-pytorch_amd.engine")
    for s in scales:
        cfg, sd, batch, c = pc.build(pc.with_sharp(pc.CASE, s))
        oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
        sdt, inp = vo.to_torch(sd), vo.to_torch(batch)
        with torch.no_grad():
            o = vo.forward(oc, sdt, inp)
            ev = o["mdl_outs_eval"]
            nz = ev != 0
            row = {"scale": s, "sharpness": eng.attention_sharpness(sd, cfg.mdl.obj_tx.n_heads, cfg.mdl.mul_tx.n_heads)}
            for label, m in plans.items():
                o2 = vo.forward(oc, sdt, inp, quant=scheme(m))
                row[label] = ((o2["mdl_outs_eval"] - ev).abs() / ev.abs().clamp(min=1e-6))[nz].max().item()
        np.savez_compressed(os.path.join(out_dir, f"x{int(s)}.npz"), mdl_outs_eval=ev.numpy(), mdl_outs=o["mdl_outs"].numpy())
        print(json.dumps(row), flush=True)


def _engine(case, tx=None):
    from tests.gpu_util import comm_for, engine_mod
    cfg, sd, batch, c = pc.build(case)
    if tx is not None:
        cfg.hip.tx_dtype = tx
    eng = engine_mod.VogEngine(cfg, comm_for(c))
    eng.load_state_dict(sd)
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    return eng, dev


def gpu(ref_dir, out_path, rounds):
    res = {"envelope": [], "timing": {}}
    for s in SCALES:
        f = os.path.join(ref_dir, f"x{int(s)}.npz")
        if not os.path.exists(f):
            continue
        ref = np.load(f)["mdl_outs_eval"]
        eng, dev = _engine(pc.with_sharp(pc.CASE, s), "split")
        ev = eng.forward(dev)["mdl_outs_eval"]
        torch.cuda.synchronize()
        ev = ev.cpu().numpy()
        nz = ref != 0
        row = {"scale": s, "sharpness": eng.sharpness, "plan": eng.plan,
               "eval_rel": float((np.abs(ev - ref)[nz] / np.maximum(np.abs(ref[nz]), 1e-6)).max()),
               "logit_max_obj_mul": eng.observed_logit_max()}
        print(json.dumps(row), flush=True)
        res["envelope"].append(row)
        del eng
    plain = dict(pc.CASE)
    plain["sharp"] = None
    runs = {"split_x16": _engine(pc.CASE, "split"), "f32_x16": _engine(pc.CASE, "f32"), "auto_f16_plain": _engine(plain)}
    slots = {}
    for k, (eng, dev) in runs.items():
        res["timing"][k] = {"plan": eng.plan, "ms": []}
        slots[k] = eng.make_slot(dev, graph=True)
        for _ in range(3):                              # warm-up of every shape
            slots[k].launch()
        torch.cuda.synchronize()
    for _ in range(rounds):
        for k, sl in slots.items():
            n, t0 = 0, time.perf_counter()
            while True:                                 # a window of at least half a second that ends in a synchronise
                for _ in range(4):
                    sl.launch()
                n += 4
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= 0.5:
                    break
            res["timing"][k]["ms"].append(1e3 * dt / n)
    B = pc.CASE["B"]
    for k, v in res["timing"].items():
        v["ms_median"] = float(np.median(v["ms"]))
        v["ms_spread"] = float(max(v["ms"]) - min(v["ms"]))
        v["queries_per_s"] = B / (v["ms_median"] * 1e-3)
        print(k, json.dumps(v), flush=True)
    t = res["timing"]
    res["split_over_f32_speedup"] = t["f32_x16"]["ms_median"] / t["split_x16"]["ms_median"]
    res["split_over_plain_throughput"] = t["auto_f16_plain"]["ms_median"] / t["split_x16"]["ms_median"]
    print(json.dumps({k: res[k] for k in ("split_over_f32_speedup", "split_over_plain_throughput")}))
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def profile(k):
    eng, dev = _engine(pc.CASE, "split")
    assert eng.plan == "split"
    for _ in range(k):
        eng.forward(dev)
    torch.cuda.synchronize()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "model":
        model(sys.argv[2], [float(x) for x in sys.argv[3:]] or SCALES)
    elif mode == "gpu":
        torch.cuda.set_device(0)
        gpu(sys.argv[2], sys.argv[3], int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3)
    else:
        torch.cuda.set_device(0)
        profile(int(sys.argv[2]))
