"""The sharp-16 p100 parity case (hi + lo operand plan at 100 proposals per frame) and the other sharpened long-sequence cases
of tests/test_split_p100_*.py.

The cases live here and not in `oracle.cases.CASES`: existing test modules build their parametrize lists from that registry
at import time. `build(case)` follows `oracle.cases.build` step by step (same generators, same order), so inputs and weights
come from the seeds and the committed fixture holds the REFERENCE outputs only, plus the SHA-256 of what was generated.

    python -m tests.p100_sharp_case        # regenerate tests/golden/full__cfg4_p100_sharp16.npz (needs the reference tree)
"""
from __future__ import annotations

import importlib
import os
import sys
import time

import numpy as np

from oracle import cases

_ec = importlib.import_module("vognet-pytorch_amd.extended_config")
_synth = importlib.import_module("vognet-pytorch_amd.synth")

NAME = "full/cfg4_p100_sharp16"
_P100 = {"mdl.name": "vog", "ds.exp_setting": "p100", **cases.REL}
# dseed 75 with relu_heavy features: few near ties among the reference's own top-1 / top-2 scores (1 frame of 520 within 1e-4
# relative, 5 within 4e-4), so the box-flip cap of max(2, 0.5 %) = 4 of 800 boxes is reachable at the modelled 5e-4 error
CASE = cases._case({**_P100, "ds.conc_type": "spat"}, B=4, nppf0=100, ragged=True, perturb_ln=True, sharp=(16.0, 4.0),
                   feat="relu_heavy", wseed=1, dseed=75)
# the other conc types at p100 (nppf = 100: four visual key blocks in mul_tx, N = 4000 in obj_tx for temp), against the CPU oracle
CASE_TEMP = cases._case({**_P100, "ds.conc_type": "temp"}, B=2, nppf0=100, ragged=True, perturb_ln=True, sharp=(16.0, 4.0),
                        feat="relu_heavy", wseed=1, dseed=76)
CASE_SEP = cases._case({**_P100, "ds.conc_type": "sep"}, B=2, nppf0=100, ragged=True, perturb_ln=True, sharp=(16.0, 4.0),
                       feat="relu_heavy", wseed=1, dseed=77)
# gt5 spat with 6 videos per query: N_obj = 300, past the 256 tokens of the gt5 hi + lo kernels
CASE_GT5_NCMP6 = cases._case({"mdl.name": "vog", "ds.conc_type": "spat", **cases.REL}, B=2, ragged=True, perturb_ln=True,
                             sharp=(16.0, 4.0), wseed=1, dseed=78, ncmp=6)


def with_sharp(case, qk):
    """The same case with wq / wk x qk (the envelope series)."""
    c = dict(case)
    c["sharp"] = (float(qk), case["sharp"][1])
    return c


def build(c):
    """-> (cfg, state_dict(np), batch(np), case), as `oracle.cases.build` does for a registered name."""
    cfg = _ec.get_default_cfg()
    _ec.update_from_dict(cfg, dict(c["over"]))
    sd = _synth.init_state_dict(cfg, c["vocab"], seed=c["wseed"], perturb_ln=c["perturb_ln"])
    msk = np.array(c["cmp_msk"], np.int64) if c.get("cmp_msk") is not None else None
    batch = _synth.make_batch(
        cfg.ds.conc_type, c["B"], c["nppf0"], ncmp=c["ncmp"], vocab_size=c["vocab"],
        prop_dim=cfg.mdl.prop_feat_dim, seg_dim=cfg.mdl.seg_feat_dim,
        seed=c["dseed"], ragged=c["ragged"], num_cmp_msk=msk, arg_lens=c.get("arg_lens"))
    if c.get("sharp"):
        cases.sharpen_state_dict(sd, *c["sharp"])
    if c.get("feat", "normal") == "relu_heavy":
        batch["pad_region_feature"] = cases.relu_heavy(batch["pad_region_feature"], c["dseed"])
        batch["seg_feature_for_frms"] = cases.relu_heavy(batch["seg_feature_for_frms"], c["dseed"] + 1)
    return cfg, sd, batch, c


def golden_path() -> str:
    return cases.golden_path(NAME)


def reference_outputs(cfg, sd, batch, c):
    """Forward + prediction head of the reference model class (CPU, fp32, eval), as oracle/make_golden.py runs them."""
    import torch
    from oracle import ref_import
    torch.set_num_threads(8)
    mdl = ref_import.build_model(cfg, c["vocab"], c["nppf0"], sd)
    inp = {k: torch.from_numpy(v).clone() for k, v in batch.items()}
    with torch.no_grad():
        out = mdl(inp)
        evl = ref_import.build_evaluator(cfg, c["nppf0"])
        inp2 = {k: torch.from_numpy(v).clone() for k, v in batch.items()}
        pr = evl.get_out_results_boxes(out, inp2)
    rec = {k: v.detach().contiguous().numpy() for k, v in out.items()}
    rec.update({k: pr[k].contiguous().numpy() for k in ("boxes", "scores", "indexs")})
    return rec


def main():
    from oracle import ref_import
    if not ref_import.available():
        raise SystemExit("reference tree not present; goldens are generated in the build container")
    cfg, sd, batch, c = build(CASE)
    t0 = time.time()
    rec = reference_outputs(cfg, sd, batch, c)
    dt = time.time() - t0
    rec["sha_inputs"] = np.array(cases.digest(batch))
    rec["sha_weights"] = np.array(cases.digest(sd))
    rec["ref_seconds"] = np.array(dt, np.float32)
    np.savez_compressed(golden_path(), **rec)
    print(f"{NAME:40s} {dt:7.2f}s  {os.path.getsize(golden_path()) / 1024:8.1f} KB")


if __name__ == "__main__":
    main()
