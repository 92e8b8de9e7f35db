"""-m gpu: whole forwards on the hi + lo operand plan at the long-sequence shapes (100 proposals per frame: obj_tx over 4000 tokens,
mul_tx layer 0 over 4 / 13 visual key blocks; gt5 spat with 6 videos per query: obj_tx over 300 tokens).

Bounds are those of tests/test_gpu_forward.py (`_check_against`: 1e-3 relative on pred_scores / mdl_outs_eval, 6e-3 abs on logits,
box flips only at near ties and at most max(2, 0.5 %) of the boxes = 4 of 800 here); the fp32 path is held to the 5e-5 / 1e-4 of
test_forward_fp32_path_vs_reference_golden."""
import numpy as np
import pytest
import torch

from tests import p100_sharp_case as pc
from tests.gpu_util import build_engine, comm_for, engine_mod, oracle_run, rel_err
from tests.test_gpu_forward import _check_against

pytestmark = pytest.mark.gpu

_BUILT = {}


def _case(key):
    import copy
    if key not in _BUILT:
        _BUILT[key] = pc.build(getattr(pc, key))
    cfg, sd, batch, c = _BUILT[key]
    return copy.deepcopy(cfg), dict(sd), dict(batch), dict(c)


def _engine(key, tx_dtype=None):
    cfg, sd, batch, c = _case(key)
    if tx_dtype is not None:
        cfg.hip.tx_dtype = tx_dtype
    eng = engine_mod.VogEngine(cfg, comm_for(c))
    eng.load_state_dict(sd)
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    return eng, cfg, sd, batch, c, dev


def _forward(eng, dev, batch, graph):
    before = {k: v.clone() for k, v in dev.items()}
    if graph:
        slot = eng.make_slot(dev, graph=True)
        slot.launch()
        torch.cuda.synchronize()
        out = slot.launch()
    else:
        out = eng.forward(dev)
    torch.cuda.synchronize()
    for k in before:                       # inputs are borrowed, never modified
        assert torch.equal(before[k], dev[k]), k
    return out, eng.unpack_pred(out["pred_rec"], batch["new_srl_idxs"].shape[1])


def test_forward_p100_sharp16_hi_lo_plan_vs_reference_golden():
    """wq / wk x 16 at 100 proposals per frame (sharpness ~ 51, past the f16 envelope) on the explicit request tx_dtype = split -
    which the parent commit refused for this model - holds the reference golden, eager and from a graph slot, bit-equal between
    the two; the logit maxima the long kernels report stay inside the plan's range. `auto` keeps the fp32 path for these models
    (engine.SPLIT_AUTO_LONG: the plan has not been timed against it)."""
    eng, *_ = _engine("CASE")
    assert eng.plan == "f32", (eng.plan, eng.sharpness)
    del eng
    eng, cfg, sd, batch, c, dev = _engine("CASE", "split")
    assert eng.plan == "split", (eng.plan, eng.sharpness)
    g = np.load(pc.golden_path())
    out, pred = _forward(eng, dev, batch, graph=False)
    _check_against(pc.NAME, out, pred, g, None, tol_rel=1e-3, tol_logit=6e-3)
    out2, pred2 = _forward(eng, dev, batch, graph=True)
    _check_against(pc.NAME, out2, pred2, g, None, tol_rel=1e-3, tol_logit=6e-3)
    assert torch.equal(out["mdl_outs"], out2["mdl_outs"])
    print(f"sharpness {eng.sharpness:.1f}, observed logit maxima (obj_tx, mul_tx): {eng.observed_logit_max()}")
    assert min(eng.observed_logit_max()) > 0          # (the long-sequence hi + lo kernels report)
    assert eng.check_logit_scale(escalate=False) is True
    assert eng.plan == "split"


@pytest.mark.parametrize("name", ["full/cfg4_vog_spat_p100_bs4", "full/cfg4_p100_sharp8"])
def test_plain_p100_cases_keep_the_f16_plan(name):
    eng, *_ = build_engine(name, cached=True)
    assert eng.plan == "f16", (eng.plan, eng.sharpness)


def test_forward_p100_sharp16_fp32_path_vs_reference_golden():
    """tx_dtype = f32 on the same case: the baseline the hi + lo plan is timed against, at a size it had never run at."""
    eng, cfg, sd, batch, c, dev = _engine("CASE", "f32")
    assert eng.plan == "f32"
    g = np.load(pc.golden_path())
    out, pred = _forward(eng, dev, batch, graph=False)
    _check_against(pc.NAME, out, pred, g, None, tol_rel=5e-5, tol_logit=1e-4)


@pytest.mark.parametrize("key,tx", [("CASE_TEMP", "split"), ("CASE_SEP", "split"), ("CASE_GT5_NCMP6", None)])
def test_forward_hi_lo_long_shapes_vs_oracle(key, tx):
    """temp / sep at 100 proposals per frame (explicit tx_dtype = split) and gt5 spat with 6 videos per query under `auto`, all
    at wq / wk x 16, against the CPU oracle: 1e-3 relative on the non-zero mdl_outs_eval."""
    eng, cfg, sd, batch, c, dev = _engine(key, tx)
    assert eng.plan == "split", (eng.plan, eng.sharpness)
    out, pred = _forward(eng, dev, batch, graph=False)
    ref = oracle_run(cfg, sd, batch, c)["mdl_outs_eval"].numpy()
    ev = out["mdl_outs_eval"].cpu().numpy()
    nz = ref != 0
    assert nz.any() and np.all(ev[~nz] == 0)
    e = float(rel_err(ev[nz], ref[nz]).max())
    print(f"{key}: mdl_outs_eval rel {e:.2e} (sharpness {eng.sharpness:.1f}, logit maxima {eng.observed_logit_max()})")
    assert e <= 1e-3, e
