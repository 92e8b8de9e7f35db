"""CPU: the oracle's restatement of LossB_TEMP / LossB_SPAT / LossB_SEP (oracle/vog_oracle.py
loss_forward) against the goldens generated from the REFERENCE loss classes (oracle/make_golden_loss.py:
tests/golden/loss__*.npz) on the reference's own forward outputs, and on perturbed ones
(tests/golden/lossperturbed__*.npz)."""
import importlib

import numpy as np
import pytest
import torch

from oracle import cases, make_golden_loss as mgl
from oracle import vog_oracle as vo


@pytest.mark.parametrize("name", mgl.LOSS_CASES)
def test_oracle_loss_vs_reference_golden(name):
    cfg, batch, c, tg = mgl.targets_for(name)
    gl = np.load(mgl.loss_path(name))
    assert str(gl["sha_targets"]) == cases.digest(tg), "target generator drifted"
    g = np.load(cases.golden_path(name))
    out = {k: torch.from_numpy(g[k]) for k in ("mdl_outs", "vidf_outs") if k in g.files}
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    res = vo.loss_forward(oc, out, vo.to_torch({**batch, **tg}), float(cfg.loss.loss_lambda))
    assert set(res) == set(gl.files) - {"sha_targets"}
    for k, v in res.items():
        assert abs(float(v) - float(gl[k])) <= 2e-6 * abs(float(gl[k])), (k, float(v), float(gl[k]))


def test_targets_are_not_trivial():
    """The synthetic ground truth must produce positive AND negative targets, masked and unmasked
    argument slots - otherwise the loss goldens would not pin the target selection."""
    cfg, batch, c, tg = mgl.targets_for("full/cfg2_vog_spat_gt5_bs4")
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    inp = vo.to_torch({**batch, **tg})
    zero = {"mdl_outs": torch.zeros(4, 1, 5, 200)}
    base = float(vo.loss_forward(oc, zero, inp)["loss"])
    assert abs(base - 200 * np.log(2.0)) < 1e-3                   # BCE at logit 0 is target independent
    ones = {"mdl_outs": torch.ones(4, 1, 5, 200)}
    l1 = float(vo.loss_forward(oc, ones, inp)["loss"])
    # all-negative targets would give 200 * softplus(1) = 262.65; positives pull it down
    assert 200 * 0.3133 < l1 < 262.6
    assert 0 < tg["srl_arg_boxes_mask"].sum() < tg["srl_arg_boxes_mask"].size


@pytest.mark.parametrize("name", mgl.PERTURBED_CASES)
def test_oracle_loss_vs_reference_live(name):
    """Away from the reference forward's own outputs: perturbed outputs and the reference loss on them
    (tests/golden/lossperturbed__*.npz, oracle/make_golden_loss.py)."""
    cfg, batch, c, tg = mgl.targets_for(name)
    g = np.load(mgl.perturbed_path(name))
    assert str(g["sha_targets"]) == cases.digest(tg), "target generator drifted"
    out = {k[len("out_"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("out_")}
    ref = {k: g[k] for k in g.files if not k.startswith(("out_", "sha_"))}
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    res = vo.loss_forward(oc, out, vo.to_torch({**batch, **tg}), float(cfg.loss.loss_lambda))
    for k in ref:
        assert abs(float(res[k]) - float(ref[k])) <= 2e-6 * abs(float(ref[k])), k
