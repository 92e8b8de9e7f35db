"""The K-split mixed-precision BiLSTM recurrence (`lstm_amp="split"`: lstm_ksplit_{fwd,bwd}_kernel<Op16>, csrc/train_lang.hip)
against the tile kernels (`lstm_amp_{fwd,bwd}_kernel`), timed alternately in one process:

  (a) the operator alone, `vog_lang_f32` forward + backward and forward only, event-timed, at the cfg-2 language shape (Bn = 4,
      T = 12, R = 1024, 2 layers; E, D, L of the cfg-2 model) and at Bn = 16, for bf16 and f16: median of `--rounds` rounds and
      their spread. The two forms differ in the 24 recurrence launches of a forward and the 24 of a backward and in nothing else,
      so (tile - split) / 24 of the forward-only call, and of the remainder, is what a launch of each new kernel saves;
  (b) the cfg-2 and cfg-5 training steps in amp bf16: the parent commit's package (`--parent DIR`: a built checkout of it), this
      tree with the default and with lstm_amp="split" - and, before anything is timed, the amp parameters after 3 steps of parent
      and default compared bit for bit.

`--trace-steps N` instead runs N tile and N split cfg-2 amp bf16 steps and nothing else, for a kernel trace taken from outside
(the per-launch time of all four recurrence kernels from one run); `--fold-trace STATS.csv` adds such a trace's rows to OUT.json.

`--vs-lib LIB.so` instead times the K-split recurrences alone (fused fp32 and split bf16; forward + backward and forward only;
Bn = 4 and 16) on another build of the library - the parent commit's - and on this tree's, each in fresh child processes that
alternate, and writes medians, spreads and a verdict per figure (profiles/train_lstm_onebody.json).

    python scratch/time_train_lstm_amp.py OUT.json [--rounds N] [--steps K] [--parent DIR] [--operator-only]
    python scratch/time_train_lstm_amp.py OUT.json --vs-lib PARENT_LIB.so [--rounds N]
"""
import csv
import importlib
import json
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
from time_train_lstm import CFG2, CFG5, _setup  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
BW = importlib.import_module("vognet-pytorch_amd.backward")
L = importlib.import_module("vognet-pytorch_amd.lib")

W16_BYTES = 2 * 4 * 1024 * 1024 * 2              # the 16-bit W_hh (or W_hh^T) of both directions at R = 1024: what a launch streams


def operator_alone(calls=10, rounds=5, modes=(("bf16", 1), ("f16", 2)), forms=("tile", "split")):
    from tests.test_gpu_train_ops import _lang_case, _lang_dev
    lib = L.load()
    sd2 = cases.build(CFG2)[1]
    E = sd2["lstm_encoder.embed_tokens.weight"].shape[1]
    R = sd2["lstm_encoder.lstm.weight_hh_l0"].shape[1]
    D, Lo = sd2["lstm_out_feat_proj.0.weight"].shape[0], sd2["srl_arg_words_out_enc.0.weight"].shape[0]
    T, layers = 12, 2
    out = {}
    for Bn in (4, 16):
        c = _lang_case(Bn, [T] * Bn, E, R, layers, D, Lo)
        for k, v in c["P"].items():                                 # nn.LSTM's scale at this fan-in (the gates do not saturate)
            if v.dim() == 2 and v.shape[1] >= 1024:
                c["P"][k] = v / 0.3 / np.sqrt(v.shape[1])
        sd, batch = _lang_dev(c)
        kw = dict(d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda())
        for mode, amp in modes:
            ms = {(form, what): [] for form in forms for what in ("fwd_bwd", "fwd")}
            try:
                lib.vog_train_set_int(b"amp", amp)
                nb = int(lib.vog_lang_f32_scratch_bytes(Bn, T, 3, E, R, layers, D, Lo))      # (one size for both forms)
                scr = torch.empty(nb, dtype=torch.uint8, device="cuda")
                for r in range(rounds + 1):                         # the forms alternate; round 0 warms up
                    for form, what in ms:
                        lib.vog_train_set_int(b"lstm_amp_split", int(form == "split"))
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(calls):
                            BW.language_backward(sd, batch, T, layers, scratch=scr, **(kw if what == "fwd_bwd" else {}))
                        e1.record()
                        torch.cuda.synchronize()
                        if r:
                            ms[(form, what)].append(e0.elapsed_time(e1) / calls)
            finally:
                lib.vog_train_set_int(b"lstm_amp_split", 0)
                lib.vog_train_set_int(b"amp", 0)
            row = {"Bn": Bn, "T": T, "E": E, "R": R, "layers": layers, "D": D, "L": Lo, "mode": mode, "scratch_bytes": nb,
                   "calls_per_timing": calls, **{f"{form}_{what}": stats(v) for (form, what), v in ms.items()}}
            med = {f"{form}_{what}": row[f"{form}_{what}"]["median"] for form, what in ms}
            if set(forms) == {"tile", "split"}:
                row["split_over_tile"] = med["split_fwd_bwd"] / med["tile_fwd_bwd"]
                row["tile_minus_split_ms"] = med["tile_fwd_bwd"] - med["split_fwd_bwd"]
                row["beyond_spread"] = bool(abs(row["tile_minus_split_ms"]) > max(row["tile_fwd_bwd"]["spread"], row["split_fwd_bwd"]["spread"]))
                n = layers * T
                row["saved_us_per_fwd_launch"] = (med["tile_fwd"] - med["split_fwd"]) / n * 1e3
                row["saved_us_per_bwd_launch"] = (row["tile_minus_split_ms"] - (med["tile_fwd"] - med["split_fwd"])) / n * 1e3
            out[f"Bn{Bn}_{mode}"] = row
            print("operator", Bn, mode, json.dumps({k: round(v, 3) for k, v in med.items()}), flush=True)
            del scr
            torch.cuda.empty_cache()
    return out


def step(name, rounds, steps, parent):
    cfg, c, sdt, dev, loss_fn = _setup(name)

    def mk(amp, **kw):
        return trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, **kw)

    summary = {"case": name, "amp": "bf16", "rounds": rounds, "steps_per_round": steps, "parent_timed": parent is not None}
    fns = {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp)
        summary["amp_params_bit_equal_to_parent_after_3_steps"] = bit_equal_after_three_steps(lambda _: mk_parent("bf16"), lambda _: mk("bf16"), dev)
        assert summary["amp_params_bit_equal_to_parent_after_3_steps"], "the default amp step differs from the parent's"
        fns["parent"] = lambda t=mk_parent("bf16"): t.step(dev)
    fns["default"] = lambda t=mk("bf16"): t.step(dev)
    fns["split"] = lambda t=mk("bf16", lstm_amp="split"): t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    if parent is not None:
        p, dflt = arms["parent"], arms["default"]
        dflt["minus_parent_median_ms"] = dflt["median"] - p["median"]
        dflt["within_parent_spread"] = bool(abs(dflt["median"] - p["median"]) <= p["spread"])
    arms["split"]["minus_default_median_ms"] = arms["split"]["median"] - arms["default"]["median"]
    arms["split"]["beyond_spread"] = bool(abs(arms["split"]["minus_default_median_ms"]) > max(arms["split"]["spread"], arms["default"]["spread"]))
    summary["arms_ms"] = arms
    losses = {m: float(fn()["loss"]) for m, fn in fns.items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    summary["loss_after"] = losses
    print(name, json.dumps({m: round(v["median"], 3) for m, v in arms.items()}), flush=True)
    return summary


def operator_child():
    """One round of the K-split recurrences on the library this process loaded (VOG_HIP_LIB, else this tree's): fused fp32 and
    split bf16, forward + backward and forward only, Bn = 4 and 16 -> one line `OPER {figure: ms}`."""
    import time_train_lstm
    torch.cuda.set_device(0)
    f32 = time_train_lstm.operator_alone(rounds=1, forms=("fused",), whats=("fwd_bwd", "fwd"))
    b16 = operator_alone(rounds=1, modes=(("bf16", 1),), forms=("split",))
    figs = {}
    for Bn in (4, 16):
        figs[f"fused_fp32/Bn{Bn}/fwd_bwd"] = f32[f"Bn{Bn}"]["fused"]["median"]
        figs[f"fused_fp32/Bn{Bn}/fwd"] = f32[f"Bn{Bn}"]["fused_fwd"]["median"]
        figs[f"split_bf16/Bn{Bn}/fwd_bwd"] = b16[f"Bn{Bn}_bf16"]["split_fwd_bwd"]["median"]
        figs[f"split_bf16/Bn{Bn}/fwd"] = b16[f"Bn{Bn}_bf16"]["split_fwd"]["median"]
    print("OPER " + json.dumps({"lib": L.LIB_PATH, "ms": figs}))


def vs_lib(other_lib, out, rounds):
    """The eight figures of operator_child on another build of the library (the parent commit's) and on this tree's: a fresh
    child process per (round, library), the libraries alternating within a round. A figure passes when the new median exceeds
    the other library's by no more than that library's own round-to-round spread (max - min) in this run."""
    import subprocess
    other_lib = os.path.abspath(other_lib)
    ms = {"parent": {}, "new": {}}
    for r in range(rounds):
        for tag in ms:
            env = {k: v for k, v in os.environ.items() if k != "VOG_HIP_LIB"}
            if tag == "parent":
                env["VOG_HIP_LIB"] = other_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "-", "--operator-child"], env=env, capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:])
                raise SystemExit(f"{tag} child of round {r} ended with {p.returncode}")
            got = json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("OPER ")][-1][5:])
            assert (got["lib"] == other_lib) == (tag == "parent"), got["lib"]
            for k, v in got["ms"].items():
                ms[tag].setdefault(k, []).append(v)
            print(r, tag, json.dumps({k: round(v, 3) for k, v in got["ms"].items()}), flush=True)
    report = {"rounds": rounds, "calls_per_timing": 10, "shape": "T = 12, R = 1024, 2 layers; E, D, L of the cfg-2 model", "figures_ms": {}}
    for k in ms["parent"]:
        p, n = stats(ms["parent"][k]), stats(ms["new"][k])
        report["figures_ms"][k] = {"parent": p, "new": n, "new_minus_parent_median": n["median"] - p["median"],
                                   "within_parent_spread": bool(n["median"] - p["median"] <= p["spread"])}
    report["all_within_parent_spread"] = all(f["within_parent_spread"] for f in report["figures_ms"].values())
    print(json.dumps({k: [round(f["parent"]["median"], 3), round(f["new"]["median"], 3), round(f["parent"]["spread"], 3),
                          f["within_parent_spread"]] for k, f in report["figures_ms"].items()}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
    return 0 if report["all_within_parent_spread"] else 1


def fold_trace(path):
    """The recurrence kernels' rows of a kernel trace's statistics file (Name, Calls, TotalDurationNs, AverageNs, ...)."""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            for key in ("lstm_ksplit_fwd", "lstm_ksplit_bwd", "lstm_amp_fwd", "lstm_amp_bwd"):   # (an amp trace: ksplit = Op16)
                if key + "_kernel" in name:
                    us = float(r["AverageNs"]) / 1e3
                    rows[key + "_kernel"] = {"calls": int(r["Calls"]), "average_us": us, "min_us": float(r["MinNs"]) / 1e3,
                                             "max_us": float(r["MaxNs"]) / 1e3, "w16_TB_per_s": W16_BYTES / us / 1e6}
    return rows


def main():
    out = sys.argv[1]
    if "--operator-child" in sys.argv:
        return operator_child()
    if "--vs-lib" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
        return vs_lib(sys.argv[sys.argv.index("--vs-lib") + 1], out, rounds)
    if "--fold-trace" in sys.argv:
        with open(out) as f:
            summary = json.load(f)
        summary["per_launch_from_kernel_trace"] = fold_trace(sys.argv[sys.argv.index("--fold-trace") + 1])
        with open(out, "w") as f:
            json.dump(summary, f, indent=1)
        return
    torch.cuda.set_device(0)
    if "--trace-steps" in sys.argv:
        cfg, c, sdt, dev, loss_fn = _setup(CFG2)
        n = int(sys.argv[sys.argv.index("--trace-steps") + 1])
        for form in ("tile", "split"):
            t = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp="bf16", lstm_amp=form)
            for _ in range(n):
                t.step(dev)
        torch.cuda.synchronize()
        return
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    summary = {"device": torch.cuda.get_device_name(0), "w16_bytes_per_launch": W16_BYTES}
    summary["operator_alone_ms"] = operator_alone(rounds=rounds)
    if "--operator-only" in sys.argv:                               # (a tiling variant's library: VOG_HIP_LIB)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1)
        return
    summary["cfg2_step"] = step(CFG2, rounds, steps, parent)
    summary["cfg5_step"] = step(CFG5, rounds, steps, parent)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
