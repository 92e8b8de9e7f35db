"""The launch-trace table of tests/test_gpu_step_trace.py: (case, tx_dtype, options, form) rows that between them take every
selection the forward's step builder makes, and the recorder of their fixture.

A row builds an engine and asks `VogEngine.describe_steps` which launches the forward would issue; nothing is launched, so a
full-size row costs its `load_state_dict` only. The fixture holds, per row, the trace, the two workspace sizes and the
(offset, bytes) of a few workspace stages: a change to the builder that moves, adds or drops a launch, or moves a buffer, shows
as a diff of the fixture.

    python -m tests.step_trace_cases        # rewrite tests/golden/step_traces.json (needs the GPU: the device weight forms
                                            # a finalized context holds decide the path)
"""
from __future__ import annotations

import ctypes as C
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_traces.json")
STAGES = ("tok", "full", "lang", "prop_seg", "obj_outA", "mul_outA16")
P100_SHARP = "full/cfg4_p100_sharp16"       # lives in tests/p100_sharp_case.py, not in oracle.cases.CASES

CFG2, CFG3, CFG5 = "full/cfg2_vog_spat_gt5_bs4", "full/cfg3_vog_temp_gt5_bs8", "full/cfg5_vog_svsq_gt5_bs16"


def _row(case, tx=None, opts=None, form="forward"):
    return {"case": case, "tx_dtype": tx, "options": dict(opts or {}), "form": form}


def row_id(r) -> str:
    o = ",".join(f"{k}={v}" for k, v in r["options"].items())
    return "|".join([r["case"], r["tx_dtype"] or "auto", o or "default", r["form"]])


ROWS = [_row(n) for n in (
    # model kinds and layouts, default options
    "small/vog_spat", "small/vog_temp", "small/vog_sep", "small/vog_svsq",
    "small/vog_spat_norel", "small/vog_spat_3layers", "small/vog_temp_objonefrm", "small/vog_spat_noobj",
    "small/vog_spat_r128", "small/vog_sep_r64", "small/vog_spat_p7",
    "small/edge_temp_len1", "small/edge_spat_b1", "small/sharp16_vgrnd_spat",
    "full/cfg1_igrnd_spat_gt5_bs2", CFG2, CFG3, "full/cfg4_vog_spat_p100_bs4", CFG5,
    "full/vgrnd_spat_gt5_bs4", "full/vog_spat_gt5_bs4_3layers",
    # hi + lo plan under `auto`
    "full/cfg2_sharp16", "full/cfg3_sharp16", "full/cfg5_sharp16")]
ROWS.append(_row(P100_SHARP, tx="split"))
for _c in (CFG2, CFG3, CFG5):
    ROWS.append(_row(_c, opts={"pair_launches": 0}))
    ROWS += [_row(_c, opts={"pair_mask": m}) for m in (1, 2, 4, 8, 7)]
    ROWS += [_row(_c, opts={"fused_ih": m}) for m in (0, 2, 3, 4, 5)]
    ROWS += [_row(_c, opts={k: 0}) for k in ("lstm_persistent", "fused_tail", "fused_enc")]
    ROWS += [_row(_c, opts={"enc_lean": m}) for m in (0, 1)]
# forms: the group language chain for 2 and 4 members, a group member, four requests batched into one slot
ROWS += [_row(CFG2, form=f) for f in ("lang2", "lang4", "member", "batched4")]

# every step name the builder can produce (the fixture-coverage test)
_TX = [f"{s}_{k}" for s in ("obj", "mul") for k in ("qkv", "attn", "tail", "wo", "ln1", "ffn1", "ffn2", "ln2")]
STEP_NAMES = (["prep", "lang_prep", "lstm_ih0", "lstm_ih1", "lstm_layer", "lstm_step", "lstm_outproj", "lstm_outproj_finish",
               "argvec", "mul_pl", "vis_prep", "vis_enc", "seg_rep", "prop_enc", "seg_enc", "enc_finish"] + _TX +
              ["mul_pv", "vislang", "lin2", "score", "pred_cmp", "pred_head",
               "lstm_layer+vis_enc", "lstm_layer+obj_tail", "lstm_outproj+mul_pv", "lstm_ih1+obj_qkv"])


_P100_ENGINE = []


def _engine(case, tx):
    """-> (engine, device inputs); engines are shared between rows (options go back to their defaults on every hand-out)."""
    from tests import gpu_util
    if case != P100_SHARP:
        eng, _, _, _, _, dev = gpu_util.build_engine(case, tx, cached=True)
        return eng, dev
    import torch
    from tests import p100_sharp_case as pc
    if not _P100_ENGINE:
        cfg, sd, batch, c = pc.build(pc.CASE)
        cfg.hip.tx_dtype = tx
        eng = gpu_util.engine_mod.VogEngine(cfg, gpu_util.comm_for(c))
        eng.load_state_dict(sd)
        _P100_ENGINE.append((eng, batch))
    eng, batch = _P100_ENGINE[0]
    return eng, {k: torch.from_numpy(v).cuda() for k, v in batch.items()}


def trace_row(r) -> dict:
    """What the fixture records for one row."""
    from tests import gpu_util
    eng, dev = _engine(r["case"], r["tx_dtype"])
    try:
        for k, v in r["options"].items():
            eng.set_option(k, v)
        form = r["form"]
        if form in ("lang2", "lang4", "member"):
            grp = eng.make_group([dev] * (4 if form == "lang4" else 2), graph=False)
            if form == "member":
                batch, ws, lang_only = grp.slots[0].batch, grp.slots[0].ws, False
            else:
                batch, ws, lang_only = grp.lb, grp.lang_ws, True
        elif form == "batched4":
            big = eng.make_batched([dev] * 4, graph=False).big
            batch, ws, lang_only = big.batch, big.ws, False
        else:
            slot = eng.make_slot(dev, graph=False)
            batch, ws, lang_only = slot.batch, slot.ws, False
        shape = (int(batch.B), int(batch.ncmp), int(batch.T))
        stages = {}
        for s in STAGES:
            off, nb = C.c_int64(), C.c_int64()
            rc = eng.lib.vog_workspace_stage(eng.ctx, *shape, s.encode(), C.byref(off), C.byref(nb))
            stages[s] = [off.value, nb.value] if rc == 0 else None
        return {"plan": eng.plan, "shape": list(shape), "trace": eng.describe_steps(batch, ws, lang_only),
                "workspace_bytes": int(eng.lib.vog_workspace_bytes(eng.ctx, *shape)),
                "lang_workspace_bytes": int(eng.lib.vog_lang_workspace_bytes(eng.ctx, *shape)), "stages": stages}
    finally:
        for k, v in gpu_util._DEFAULT_OPTIONS.items():
            eng.set_option(k, v)


def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def main():
    rec = {}
    for r in ROWS:
        rec[row_id(r)] = trace_row(r)
        print(f"{row_id(r):80s} {len(rec[row_id(r)]['trace']):3d} launches", flush=True)
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{FIXTURE}: {len(rec)} rows, {os.path.getsize(FIXTURE) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
