"""CPU: the autograd path's host side (autograd.py) - which parameters are the Function's inputs, and that the
default state of a model never enters it."""
import importlib

import numpy as np
import pytest
import torch

from oracle import cases
from oracle import make_golden_bwd as mgb
from tests.gpu_util import comm_for

AG = importlib.import_module("vognet-pytorch_amd.autograd")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")


@pytest.mark.parametrize("name", ["small/igrnd_spat", "small/vgrnd_temp", "small/vgrnd_sep", "small/vog_spat", "small/vog_temp",
                                  "small/vog_spat_noobj", "small/vog_spat_norel", "small/vog_sep_cmpmsk"])
def test_used_parameters_are_the_ones_the_reference_differentiates(name):
    """The parameters handed to the autograd Function (those the device forward reads) cover every float state-dict key
    but the ones the reference's forward never reads, and are exactly the parameters the reference's `loss.backward()`
    gives a gradient to (tests/golden/bwd__*.npz `p:` keys; plus the sep verb head, which only verb_loss reaches)."""
    cfg, sd, batch, c = cases.build(name)
    mdl = sel_mod.get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm_for(c))
    names = [n for n, p in mdl.named_parameters() if p.is_floating_point()]
    assert set(names) == {k for k, v in mdl.state_dict().items() if v.is_floating_point()}
    used = set(AG.used_param_names(cfg, comm_for(c), names))
    g = np.load(mgb.bwd_path(name))
    have = {k[2:-len("__shape")] for k in g.files if k.startswith("p:") and k.endswith("__shape")}
    verb = {n for n in names if n.startswith("seg_verb_classf.")} if cfg.ds.conc_type in ("sep", "svsq") else set()
    assert used == have | verb, used ^ (have | verb)


def test_default_state_and_no_grad_stay_on_the_inference_path():
    cfg, sd, batch, c = cases.build("small/vog_spat")
    mdl = sel_mod.get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm_for(c))
    inp = {k: torch.from_numpy(v) for k, v in batch.items()}
    assert not any(p.requires_grad for p in mdl.parameters())
    assert not AG.wants_grad(mdl, inp)
    mdl.requires_grad_(True)
    assert AG.wants_grad(mdl, inp)
    with torch.no_grad():
        assert not AG.wants_grad(mdl, inp)
    mdl.requires_grad_(False)
    inp["pad_region_feature"] = inp["pad_region_feature"].float().requires_grad_(True)
    assert AG.wants_grad(mdl, inp)
