"""Oracle <-> reference on the reference's stored outputs.

tests/golden/<case>.npz hold what the reference's forward + prediction head return for each case
(oracle/make_golden.py); tests/golden/refmask__small__vog_spat.npz the input mask its forward leaves behind."""
import numpy as np
import pytest
import torch

from oracle import cases, make_golden as mg
from oracle import vog_oracle as vo


def _reference_outputs(name, batch, sd):
    """Every array the reference's forward + prediction head returned for `name`, as stored by oracle/make_golden.py."""
    g = np.load(cases.golden_path(name))
    assert str(g["sha_inputs"]) == cases.digest(batch), "synthetic input generator drifted"
    assert str(g["sha_weights"]) == cases.digest(sd), "weight generator drifted"
    return {k: g[k] for k in g.files if not k.startswith(("st_", "sha_")) and k != "ref_seconds"}


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep", "small/vgrnd_temp",
                                  "small/igrnd_svsq", "full/cfg2_vog_spat_gt5_bs4"])
def test_live(name):
    cfg, sd, batch, c = cases.build(name)
    ref = _reference_outputs(name, batch, sd)
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    inp = vo.to_torch(batch)
    with torch.no_grad():
        out = vo.forward(oc, vo.to_torch(sd), inp)
        out.update(vo.pred_head(oc, out, inp))
    for k, v in ref.items():
        np.testing.assert_allclose(out[k].float().numpy(), v.astype(np.float32), atol=2e-5, rtol=0,
                                   err_msg=k)


def test_reference_mutates_mask_oracle_does_not():
    """the reference overwrites -1 -> 0 in srl_arg_word_mask."""
    cfg, sd, batch, c = cases.build(mg.MASK_CASE)
    g = np.load(mg.mask_path())
    assert str(g["sha_inputs"]) == cases.digest(batch), "synthetic input generator drifted"
    ref_mask = g["srl_arg_word_mask_after_forward"]
    assert (ref_mask >= 0).all()
    assert (batch["srl_arg_word_mask"] < 0).any()
    assert np.array_equal(ref_mask, np.maximum(batch["srl_arg_word_mask"], 0))
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    inp = vo.to_torch(batch)
    before = inp["srl_arg_word_mask"].clone()
    with torch.no_grad():
        vo.forward(oc, vo.to_torch(sd), inp)
    assert torch.equal(inp["srl_arg_word_mask"], before)
