"""The fused fp32 BiLSTM recurrence (`lstm="fused"`: lstm_ksplit_{fwd,bwd}_kernel<OpF32>, csrc/train_lang.hip) against the stepwise one,
timed alternately in one process:

  (a) the operator alone, `vog_lang_f32` forward + backward, event-timed, at the cfg-2 language shape (Bn = 4, T = 12, R = 1024,
      2 layers; E, D, L of the cfg-2 model) and at Bn = 16;
  (b) the cfg-2 and cfg-5 training steps in fp32, median of `--rounds` rounds of `--steps` steps with the spread: the parent
      commit's package (`--parent DIR`: a built checkout of it), this tree with the default, lstm="fused" and, at cfg 2,
      lstm="fused" with attn="fused" - and, before anything is timed, the fp32 parameters after 3 steps of parent and default
      compared bit for bit;
  (c) the deviations from float64 at the model's width of both paths (tests/test_gpu_train_lstm.py::width_deviations).

`--trace-steps N` instead runs N fused cfg-2 steps and nothing else (for a kernel trace taken from outside).

    python scratch/time_train_lstm.py OUT.json [--rounds N] [--steps K] [--parent DIR]
"""
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

trn = importlib.import_module("vognet-pytorch_amd.train")
BW = importlib.import_module("vognet-pytorch_amd.backward")
L = importlib.import_module("vognet-pytorch_amd.lib")
synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")

CFG2, CFG5 = "full/cfg2_vog_spat_gt5_bs4", "full/cfg5_vog_svsq_gt5_bs16"


def operator_alone(calls=10, rounds=5, forms=("stepwise", "fused"), whats=("fwd_bwd",)):
    """`forms` x `whats` (forward + backward | forward only) alternate within a round; a row's keys are the form's name for
    fwd_bwd and FORM_fwd for the forward alone. (One form, both whats, one round: a child of time_train_lstm_amp.py --vs-lib.)"""
    from tests.test_gpu_train_ops import _lang_case, _lang_dev
    lib = L.load()
    sd2 = cases.build(CFG2)[1]
    E = sd2["lstm_encoder.embed_tokens.weight"].shape[1]
    R = sd2["lstm_encoder.lstm.weight_hh_l0"].shape[1]
    D, Lo = sd2["lstm_out_feat_proj.0.weight"].shape[0], sd2["srl_arg_words_out_enc.0.weight"].shape[0]
    out = {}
    for Bn in (4, 16):
        c = _lang_case(Bn, [12] * Bn, E, R, 2, D, Lo)
        for k, v in c["P"].items():                                 # nn.LSTM's scale at this fan-in (the gates do not saturate)
            if v.dim() == 2 and v.shape[1] >= 1024:
                c["P"][k] = v / 0.3 / np.sqrt(v.shape[1])
        sd, batch = _lang_dev(c)
        kw = dict(d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda())
        ms, nb, scr = {(form, what): [] for form in forms for what in whats}, {}, {}
        for form in forms:
            lib.vog_train_set_int(b"lstm_fused", int(form == "fused"))
            nb[form] = int(lib.vog_lang_f32_scratch_bytes(Bn, 12, 3, E, R, 2, D, Lo))
            scr[form] = torch.empty(nb[form], dtype=torch.uint8, device="cuda")
        try:
            for r in range(rounds + 1):                             # the forms alternate; round 0 warms up
                for form, what in ms:
                    lib.vog_train_set_int(b"lstm_fused", int(form == "fused"))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        BW.language_backward(sd, batch, 12, 2, scratch=scr[form], **(kw if what == "fwd_bwd" else {}))
                    e1.record()
                    torch.cuda.synchronize()
                    if r:
                        ms[(form, what)].append(e0.elapsed_time(e1) / calls)
        finally:
            lib.vog_train_set_int(b"lstm_fused", 0)
        row = {"Bn": Bn, "T": 12, "E": E, "R": R, "layers": 2, "D": D, "L": Lo, "scratch_bytes": nb, "calls_per_timing": calls,
               **{form if what == "fwd_bwd" else f"{form}_{what}": stats(v) for (form, what), v in ms.items()}}
        if "stepwise" in row and "fused" in row:
            row["fused_over_stepwise"] = row["fused"]["median"] / row["stepwise"]["median"]
        out[f"Bn{Bn}"] = row
        print("operator", Bn, json.dumps({k: round(v["median"], 3) for k, v in row.items() if isinstance(v, dict) and "median" in v}), flush=True)
        del scr
        torch.cuda.empty_cache()
    return out


def _setup(name):
    cfg, sd, batch, c = cases.build(name)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    return cfg, c, sdt, dev, sel["loss"](cfg, comm_for(c))


def step(name, rounds, steps, parent, with_attn):
    cfg, c, sdt, dev, loss_fn = _setup(name)

    def mk(amp, **kw):
        return trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, **kw)

    summary = {"case": name, "rounds": rounds, "steps_per_round": steps, "parent_timed": parent is not None}
    fns = {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp)
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = bit_equal_after_three_steps(mk_parent, mk, dev)
        fns["parent"] = lambda t=mk_parent(None): t.step(dev)
    fns["default"] = lambda t=mk(None): t.step(dev)
    fns["lstm_fused"] = lambda t=mk(None, lstm="fused"): t.step(dev)
    if with_attn:
        fns["attn_fused"] = lambda t=mk(None, attn="fused"): t.step(dev)
        fns["lstm_fused+attn_fused"] = lambda t=mk(None, lstm="fused", attn="fused"): t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    if parent is not None:
        p, dflt = arms["parent"], arms["default"]
        dflt["minus_parent_median_ms"] = dflt["median"] - p["median"]
        dflt["within_parent_spread"] = bool(abs(dflt["median"] - p["median"]) <= p["spread"])
    arms["lstm_fused"]["minus_default_median_ms"] = arms["lstm_fused"]["median"] - arms["default"]["median"]
    summary["arms_ms"] = arms
    losses = {m: float(fn()["loss"]) for m, fn in fns.items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    summary["loss_after"] = losses
    print(name, json.dumps({m: round(v["median"], 3) for m, v in arms.items()}), flush=True)
    return summary


def main():
    torch.cuda.set_device(0)
    if "--trace-steps" in sys.argv:
        cfg, c, sdt, dev, loss_fn = _setup(CFG2)
        t = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, lstm="fused")
        for _ in range(int(sys.argv[sys.argv.index("--trace-steps") + 1])):
            t.step(dev)
        torch.cuda.synchronize()
        return
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    summary = {"device": torch.cuda.get_device_name(0)}
    summary["operator_alone_ms"] = operator_alone()
    summary["cfg2_step"] = step(CFG2, rounds, steps, parent, True)
    summary["cfg5_step"] = step(CFG5, rounds, steps, parent, False)
    from tests.test_gpu_train_lstm import WIDE_4, WIDE_16, width_deviations
    summary["width_deviations"] = {
        tag: {k: {"stepwise": e0, "fused": e1, "bound_for_fused": b} for k, (e0, e1, b) in width_deviations(key).items()}
        for tag, key in (("Bn4", WIDE_4), ("Bn16", WIDE_16))}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
