"""Bits of the trainer against another build of the library (train_dedupe, train_lstm_onebody, opt_onebody: merged kernels against
the parent's).

    python scratch/bits_vs_parent.py PARENT_LIB.so OUT.json      # PARENT_LIB: libvog_hip.so built from the parent commit
    python scratch/bits_vs_parent.py --child                     # (one child process per library, selected with VOG_HIP_LIB)

Each child runs, on small/vog_spat, three steps in each of MODES (fp32 and bf16 with a dynamic loss scale; the K-split BiLSTM
recurrences: lstm="fused" in fp32, lstm_amp="split" in bf16 and in f16 with a dynamic loss scale; the optimiser's modes: clipping,
AdamW with a weight-decay group, AMSGrad, an accumulation window of two with a flush behind the last step, EMA averaging), and on
small/vog_sep_cmpmsk (d_hid / final_hidden) one step of each, and prints the SHA-256 of every parameter, both Adam moments, vmax,
the averages and the loss dict of every step, with the scaler state, the f32_products counter and the two recurrence launch
counters. The parent process compares the two listings entry by entry."""
import ctypes
import hashlib
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RUNS = [("small/vog_spat", 3), ("small/vog_sep_cmpmsk", 1)]
MODES = {"fp32": {}, "bf16_dynamic_scale": {"amp": "bf16", "loss_scale": "dynamic"},
         "fp32_lstm_fused": {"lstm": "fused"}, "bf16_lstm_split": {"amp": "bf16", "lstm_amp": "split"},
         "f16_lstm_split_dynamic_scale": {"amp": "f16", "lstm_amp": "split", "loss_scale": "dynamic"},
         "clip_norm_1": {"clip_norm": 1.0}, "adamw_decay_group": {"optimizer": "adamw", "param_groups": "halves"},
         "amsgrad": {"amsgrad": True}, "accum_2": {"accum_steps": 2}, "avg_ema": {"avg": "ema"}}
COUNTERS = ("f32_products", "lstm_fused_launches", "lstm_amp_split_launches")


def child():
    import numpy as np
    import torch
    from oracle import cases
    from tests.gpu_util import comm_for
    trn = importlib.import_module("vognet-pytorch_amd.train")
    L = importlib.import_module("vognet-pytorch_amd.lib")
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    out = {"lib": L.LIB_PATH}
    lib = L.load()
    for name, steps in RUNS:
        cfg, sd, batch, c = cases.build(name)
        tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
        sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
        loss_fn = sel_mod.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))
        names = sorted(sdt)
        halves = [{"params": names[:len(names) // 2], "weight_decay": 0.01}, {"params": names[len(names) // 2:]}]
        for mode, kw in MODES.items():
            kw = {k: halves if v == "halves" else v for k, v in kw.items()}
            tr = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, **kw)
            for cn in COUNTERS:
                assert lib.vog_train_set_int(cn.encode(), 0) == 0
            rec = {}
            for s in range(steps):
                ld = tr.step(dev)
                rec[f"step{s}/loss"] = {k: sha(v) if torch.is_tensor(v) else repr(v) for k, v in sorted(ld.items())}
            tr.flush()                                               # (the open window of accum_steps = 2; a no-op otherwise)
            torch.cuda.synchronize()
            for cn in COUNTERS:
                n32 = ctypes.c_int32(-1)
                assert lib.vog_train_get_int(cn.encode(), ctypes.byref(n32)) == 0
                rec[cn] = n32.value
            rec["scaler"] = repr(sorted(tr.scaler_state().items()))
            rec["loss_last"] = float(ld["loss"])
            for k in sorted(tr.params):
                rec["p/" + k] = sha(tr.params[k])
            for k in sorted(tr.m):
                rec["m/" + k], rec["v/" + k] = sha(tr.m[k]), sha(tr.v[k])
            for tag, held in (("vmax/", tr.vmax), ("avg/", tr.avg)):
                for k in sorted(held):
                    rec[tag + k] = sha(held[k])
            out[f"{name}/{mode}"] = rec
    print("BITS " + json.dumps(out))


def main():
    if "--child" in sys.argv:
        return child()
    parent_lib, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    got = {}
    for tag, env in (("parent", {"VOG_HIP_LIB": parent_lib}), ("new", {})):
        e = {k: v for k, v in os.environ.items() if k != "VOG_HIP_LIB"}
        e.update(env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=e, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:])
            raise SystemExit(f"{tag} child ended with {r.returncode}")
        got[tag] = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("BITS ")][-1][5:])
    assert got["parent"].pop("lib") == parent_lib and got["new"].pop("lib") != parent_lib
    report, ok = {}, True
    for run in got["parent"]:
        a, b = got["parent"][run], got["new"][run]
        diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        report[run] = {"entries": len(a), **{cn: [a[cn], b[cn]] for cn in COUNTERS}, "loss_last": [a["loss_last"], b["loss_last"]],
                       "scaler": b["scaler"], "differing_entries": diff}
        ok = ok and not diff
    report["byte_equal"] = ok
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
