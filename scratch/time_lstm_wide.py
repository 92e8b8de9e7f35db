"""The wide persistent BiLSTM layer kernel (vog_bilstm_layer_wide, context option "lstm_wide": 17 .. 32 sentences) against the
step-launch form it replaces, everything in one process with the forms alternated, median of `--rounds` rounds with the spread:

  (a) per layer, event-timed at R = 1024: one wide launch (gxs form, gate-table form) against the T vog_bilstm_step launches,
      Bn in {17, 24, 32} x T in {12, 20}; the narrow kernel at Bn = 16 as the anchor. Every timed call re-arms its buffers the
      way the forward's prologue does (out16 / state zero, hand-off slots 0xffff); the arming alone is timed the same way and
      reported next to it (`minus_arm` = the difference).
  (b) forward-only replay of captured slots (one forward in flight, graph launches back to back, one synchronise per window),
      option off against on: cfg-2 dimensions at spat B = 32, sep B = 8, svsq B = 32, and make_batched of eight bs-4 requests.
  (c) no movement: the default (option off) at cfg 2 / bs = 4 against the parent commit's package (`--parent DIR`: a built
      checkout of it), alternated; `within_parent_spread` says whether the medians differ by less than the parent's own spread.

    python scratch/time_lstm_wide.py OUT.json [--rounds N] [--steps K] [--parent DIR]
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
from tests import lstm_ref as lr  # noqa: E402
from tests.gpu_util import comm_for  # noqa: E402

L = importlib.import_module("vognet-pytorch_amd.lib")
E = importlib.import_module("vognet-pytorch_amd.engine")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
synth = importlib.import_module("vognet-pytorch_amd.synth")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "spread": float(np.max(v) - np.min(v)), "all": v}


def _p(t):
    return C.c_void_p(t.data_ptr())


# ---- (a) one layer -----------------------------------------------------------------------------------------------------------
def layer_forms(Bn, T, R=1024, dtype="f16"):
    """-> {form: callable that arms and launches one layer}, {form: callable that only arms}"""
    lib = L.load()
    dt = L.VOG_F16 if dtype == "f16" else L.VOG_BF16
    lens = lr.make_lens("mix", Bn, T)
    lens = [max(ln, T - 2) for ln in lens]                       # near-full sentences: the time of a layer is its longest sentence's
    lens_d = torch.tensor(lens, dtype=torch.int64).cuda()
    whh = lr.pack_w(lib, lr.rand_whh(R), R, R, dt).cuda()
    gxs = lr.make_gxs(lr.rand_gx(Bn, T, R, 1), lens).nan_to_num(0.0).cuda()
    table, tok, _ = lr.make_table(lr.TABLE_V, R, Bn, T, lens, 2)
    table, tok = table.cuda(), tok.cuda()
    rows = (Bn * T + Bn + 15) // 16 * 16
    Bn16 = (Bn + 15) // 16 * 16
    out16 = torch.zeros(rows * 2 * R, dtype=torch.int16, device="cuda")
    hx = torch.empty(int(lib.vog_bilstm_hx_bytes(Bn, T, R)), dtype=torch.uint8, device="cuda")
    sync = torch.zeros(256, dtype=torch.int32, device="cuda")
    fault = torch.zeros(1, dtype=torch.int32, device="cuda")
    h = [torch.zeros(Bn16 * 2 * R, dtype=torch.int16, device="cuda") for _ in range(2)]
    c = torch.zeros(Bn16 * 2 * R, dtype=torch.float32, device="cuda")
    keep = [lens_d, whh, gxs, table, tok, out16, hx, sync, fault, h, c]

    def layer_args(tab):
        a = L.LstmLayerArgs()
        a.lens, a.whh, a.hx, a.sync, a.out16, a.fault = _p(lens_d), _p(whh), _p(hx), _p(sync), _p(out16), _p(fault)
        a.Bn, a.T, a.R, a.dtype, a.out_frag, a.inject_stall = Bn, T, R, dt, 0, 0
        if tab:
            a.gx_table, a.tok = _p(table), _p(tok)
        else:
            a.gxs = _p(gxs)
        return a

    sa = L.LstmStepArgs()
    sa.gx, sa.whh, sa.c, sa.out16, sa.lens = _p(gxs), _p(whh), _p(c), _p(out16), _p(lens_d)
    sa.Bn, sa.T, sa.R, sa.dtype, sa.out_frag, sa.final_row0 = Bn, T, R, dt, 0, Bn * T
    entry = lib.vog_bilstm_layer if Bn <= 16 else lib.vog_bilstm_layer_wide
    a_gxs, a_tab = layer_args(False), layer_args(True)

    def arm_layer():
        out16.zero_(); hx.fill_(0xff); sync.zero_()

    def arm_steps():
        out16.zero_(); h[0].zero_(); c.zero_()

    def run_layer(a):
        arm_layer()
        L.check(entry(C.byref(a), L.stream_ptr()), "layer")

    def run_steps():
        arm_steps()
        for s in range(T):
            sa.step, sa.h_in, sa.h_out = s, _p(h[s & 1]), _p(h[(s + 1) & 1])
            L.check(lib.vog_bilstm_step(C.byref(sa), L.stream_ptr()), "step")

    forms = {"layer_gxs": lambda: run_layer(a_gxs), "layer_table": lambda: run_layer(a_tab), "steps": run_steps}
    arms = {"layer_gxs": arm_layer, "layer_table": arm_layer, "steps": arm_steps}
    return forms, arms, keep, (sync, fault)


def event_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def per_layer(rounds, calls=40):
    out = {}
    for Bn, T in [(16, 12), (16, 20)] + [(Bn, T) for Bn in (17, 24, 32) for T in (12, 20)]:
        forms, arms, keep, (sync, fault) = layer_forms(Bn, T)
        us = {k: [] for k in forms}
        arm_us = {k: [] for k in forms}
        for r in range(rounds + 1):                              # round 0 warms up; the forms alternate
            for k in forms:
                a, b = event_us(forms[k], calls), event_us(arms[k], calls)
                if r:
                    us[k].append(a)
                    arm_us[k].append(b)
        assert int(sync[2]) == 0 and int(fault[0]) == 0, "a hand-off timed out while timing"
        row = {"Bn": Bn, "T": T, "R": 1024, "calls_per_timing": calls}
        for k in forms:
            row[k] = stats(us[k])
            row[k]["arm_alone"] = stats(arm_us[k])
            row[k]["minus_arm"] = row[k]["median"] - row[k]["arm_alone"]["median"]
            row[k]["per_step_minus_arm"] = row[k]["minus_arm"] / T
        for k in ("layer_gxs", "layer_table"):
            row[k]["over_steps"] = row[k]["minus_arm"] / row["steps"]["minus_arm"]
        out[f"Bn{Bn}_T{T}"] = row
        print("layer", Bn, T, json.dumps({k: round(row[k]["minus_arm"], 1) for k in forms}), flush=True)
        del forms, arms, keep
        torch.cuda.empty_cache()
    return out


# ---- (b) forward-only slot replay ------------------------------------------------------------------------------------------
REL = cases.REL


def full_case(conc, B, dseed):
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"mdl.name": "vog", "ds.conc_type": conc, **REL})
    c = {"vocab": 5000, "nppf0": 5}
    sd = synth.init_state_dict(cfg, 5000, seed=1)
    batch = synth.make_batch(conc, B, 5, ncmp=4, vocab_size=5000, prop_dim=cfg.mdl.prop_feat_dim, seg_dim=cfg.mdl.seg_feat_dim,
                             seed=dseed, ragged=True)
    return cfg, c, sd, batch


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def to_dev(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}


def replay(tag, conc, B, rounds, steps, batched=0):
    cfg, c, sd, batch = full_case(conc, B, 7)
    eng = E.VogEngine(cfg, comm_for(c))
    eng.load_state_dict(sd)
    arms, traces = {}, {}
    for opt in (0, 1):
        eng.set_option("lstm_wide", opt)
        if batched:
            inps = [to_dev(full_case(conc, B, 20 + i)[3]) for i in range(batched)]
            T = max(int(i["srl_arg_word_mask_len"].max()) for i in inps)
            arms[opt] = eng.make_batched(inps, graph=True)
        else:
            dev = to_dev(batch)
            arms[opt] = eng.make_slot(dev, graph=True)
            b, _, (B_, ncmp, T) = eng.make_batch(dev)
            traces[opt] = eng.describe_steps(b, eng.workspace(B_, ncmp, T))
    eng.set_option("lstm_wide", 0)
    res = {0: [], 1: []}
    for _ in range(rounds):
        for opt in (0, 1):
            res[opt].append(timed(arms[opt].launch, steps))
    for opt in (0, 1):
        arms[opt].check()
    # (the two forms of the recurrence sum in another order: what the timed forwards computed must agree to logit tolerance)
    diff = None
    if not batched:
        outs = []
        for opt in (0, 1):
            o = arms[opt].launch()
            torch.cuda.synchronize()
            outs.append(o["mdl_outs"].clone())
        diff = float((outs[0] - outs[1]).abs().max())
        assert bool(torch.isfinite(outs[1]).all()) and diff < 1.5e-3, (tag, diff)
    nq = B * (batched or 1)
    off, on = stats(res[0]), stats(res[1])
    row = {"case": tag, "queries_per_forward": nq, "rounds": rounds, "steps_per_round": steps, "T": T,
           "off_ms": off, "on_ms": on, "off_queries_per_s": nq / off["median"] * 1e3, "on_queries_per_s": nq / on["median"] * 1e3,
           "on_over_off_time": on["median"] / off["median"]}
    if traces:
        row["launches_off"], row["launches_on"], row["logits_max_abs_diff_on_vs_off"] = len(traces[0]), len(traces[1]), diff
    print("replay", tag, json.dumps({k: round(v, 3) for k, v in row.items() if isinstance(v, float)}), flush=True)
    del arms, eng
    torch.cuda.empty_cache()
    return row


# ---- (c) the default against the parent commit -------------------------------------------------------------------------------
def load_parent_engine(path):
    pkg = os.path.join(path, "vognet-pytorch_amd")
    spec = importlib.util.spec_from_file_location("vog_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vog_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("vog_parent.engine")


def no_movement(parent_dir, rounds, steps):
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sd, batch, c = cases.build(name)
    slots, engs = {}, {}
    for tag, mod in (("parent", load_parent_engine(parent_dir)), ("default", E)):
        engs[tag] = mod.VogEngine(cfg, comm_for(c))
        engs[tag].load_state_dict(sd)
        slots[tag] = engs[tag].make_slot(to_dev(batch), graph=True)
    outs = {}
    for tag in slots:
        o = slots[tag].launch()
        torch.cuda.synchronize()
        outs[tag] = {k: o[k].clone() for k in ("mdl_outs", "pred_rec")}
    equal = all(torch.equal(outs["parent"][k], outs["default"][k]) for k in outs["parent"])
    res = {t: [] for t in slots}
    for _ in range(rounds):
        for t in slots:
            res[t].append(timed(slots[t].launch, steps))
    p, d = stats(res["parent"]), stats(res["default"])
    row = {"case": name, "rounds": rounds, "steps_per_round": steps, "outputs_bit_equal_to_parent": bool(equal), "parent_ms": p, "default_ms": d,
           "default_minus_parent_median_ms": d["median"] - p["median"], "within_parent_spread": bool(abs(d["median"] - p["median"]) <= p["spread"])}
    print("no movement", json.dumps({k: v for k, v in row.items() if not isinstance(v, dict)}), flush=True)
    return row


def main():
    torch.cuda.set_device(0)
    out = sys.argv[1]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 100
    summary = {"device": torch.cuda.get_device_name(0), "rounds": rounds}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1)

    summary["per_layer_us"] = per_layer(rounds)
    save()
    summary["slot_replay"] = [replay("cfg2_spat_B32", "spat", 32, rounds, steps), replay("sep_B8", "sep", 8, rounds, steps),
                              replay("svsq_B32", "svsq", 32, rounds, steps),
                              replay("cfg2_spat_8x_bs4_batched", "spat", 4, rounds, steps, batched=8)]
    save()
    if "--parent" in sys.argv:
        summary["no_movement"] = no_movement(sys.argv[sys.argv.index("--parent") + 1], rounds, steps)
    save()


if __name__ == "__main__":
    main()
