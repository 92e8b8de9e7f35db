"""CPU: the loss at the branches the 14 loss goldens never reach (tests/loss_ref.py), without a device.

(1) The oracle against the REFERENCE LossB_* on those inputs (tests/golden/lossedge__*.npz, oracle/make_golden_loss.make_edge;
the inputs come back from the seed, their SHA pins the generator): the fp32 oracle within the 2e-6 of test_loss_oracle.py, NaN
where the reference is NaN, and the float64 autograd gradient of the oracle - what tests/test_gpu_loss_ops.py holds the
kernels to - within 1e-6 + 2e-5 max|ref| of the reference's autograd gradient.
(2) Conditions on the inputs, so that no device test passes vacuously: every case reaches the branch it is named for."""
import math

import numpy as np
import pytest

from oracle import make_golden_loss as mgl
from tests import loss_ref as lr


def _ref(name, _cache={}):
    if name not in _cache:
        case, lam = lr.build(name)
        r = lr.ref64(case, lam)
        _cache[name] = (case, lam, r, lr.stats(case, r))
    return _cache[name]


def test_every_case_but_the_large_one_has_a_fixture():
    assert set(mgl.EDGE_CASES) == set(lr.CASES) - {"stride_spat_313"}


@pytest.mark.parametrize("name", mgl.EDGE_CASES)
def test_oracle_vs_reference_on_edge_inputs(name):
    case, lam, r64, _ = _ref(name)
    g = np.load(mgl.edge_path(name))
    assert str(g["sha_inputs"]) == lr.digest_of(case), "make_case drifted"
    o32 = lr.oracle32(case, lam)
    keys = {"loss", "mdl_out_loss"} | ({"verb_loss"} if case["conc"] == "sep" else set())
    assert set(o32) == keys and keys <= set(g.files)
    for k in keys:
        ref = float(g[k])
        if math.isnan(ref):
            assert math.isnan(o32[k]) and math.isnan(r64[k]), (k, o32[k], r64[k])
        else:
            assert abs(o32[k] - ref) <= 2e-6 * abs(ref), (k, o32[k], ref)
    for k in ("grad_mdl_outs", "grad_vidf_outs")[:2 if case["conc"] == "sep" else 1]:
        ref = g[k].astype(np.float64)
        assert np.isfinite(ref).all() and np.isfinite(r64[k]).all()
        err, bound = float(np.abs(r64[k] - ref).max()), 1e-6 + 2e-5 * float(np.abs(ref).max())
        print(f"    {name} {k}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (k, err, bound)
    assert not r64["grad_mdl_outs"][~r64["in_mean"]].any() and not g["grad_mdl_outs"][~r64["in_mean"]].any()


@pytest.mark.parametrize("name", lr.THRESHOLD)
def test_threshold_cases_reach_their_branches(name):
    case, lam, r, s = _ref(name)
    print("   ", name, s)
    assert r["masked"] and s["n_pos"] > 0
    assert s["gathered_empty_gt"] > 0 and s["empty_props_on_target"] > 0 and s["gathered_empty_prop"] > 0
    assert s["flip_exact_half"] > 0 and s["just_above"] > 0 and s["exact_half"] >= s["flip_exact_half"]
    assert s["flip_without_empty_gt_rule"] > 0 and s["flip_without_empty_prop_rule"] > 0
    assert s["near_half"] == 0
    # the copies of the edge proposals in a non-target video, and everything else there, have target 0
    tg, info = lr.gathered(case)
    assert not (r["targets"] & ~np.broadcast_to(info["on"][..., 0], r["targets"].shape)).any()
    # lens = 0 on the only box above 1/2 (pattern C): some element in the mean would be positive with that lens set
    full = {**case, "inp": {**case["inp"], "srl_boxes_lens": np.ones_like(case["inp"]["srl_boxes_lens"])}}
    assert ((lr.gathered(full)[0].max(-1) > 0.5) & ~r["targets"] & r["in_mean"]).any()


@pytest.mark.parametrize("name", sorted(set(lr.CASES) - set(lr.THRESHOLD)))
def test_no_case_sits_near_the_threshold(name):
    assert _ref(name)[3]["near_half"] == 0


@pytest.mark.parametrize("name", lr.PLAIN)
def test_plain_mean_cases_tell_the_two_means_apart(name):
    case, lam, r, s = _ref(name)
    assert not r["masked"] and r["n_mean"] == case["out"]["mdl_outs"].size
    plain, masked = r["mean_plain"], r["mean_masked"]
    assert abs(r["loss"] - plain * case["out"]["mdl_outs"].shape[-1] * lam) <= 1e-12 * abs(r["loss"])
    if case["conc"] == "sep":
        assert abs(plain - masked) > 1e-3 * abs(plain), (plain, masked)
    else:
        assert math.isnan(masked)                     # every bm is 0: the masked mean would be 0 / 0
    # the gradient reaches elements the masked mean would leave out (temp / spat), scaled by the video mask (sep)
    cm = case["inp"]["num_cmp_msk"]
    assert (cm == 0).any() and (cm != 0).any()
    g = r["grad_mdl_outs"]
    if case["conc"] == "sep":
        assert (g[cm == 0] == 0).all() and (g[cm != 0] != 0).all()
    else:
        assert (g != 0).all()


def test_stride_cases_need_the_stride():
    case, lam, r, _ = _ref("stride_spat_313")
    assert (case["out"]["mdl_outs"].size + 255) // 256 == 313
    case, lam, r, _ = _ref("stride_abm_260")
    abm = case["inp"]["srl_arg_boxes_mask"].reshape(-1)
    assert abm.size == 260 and abm[-1] == 1 and not abm[:-1].any() and r["masked"]
    assert abs(r["mean_plain"] - r["mean_masked"]) > 1e-3 * abs(r["mean_masked"])
    case, lam, r, _ = _ref("stride_verb_260")
    vm = case["inp"]["verb_cross_cmp_msk"].reshape(260, -1)
    assert not vm[:256].any() and not vm[:, :-1].any() and vm[256:, -1].all() and r["n_verb"] == 4
    assert [lr.build(n)[0]["out"]["mdl_outs"].size for n in ("tot_3", "tot_64", "tot_256", "tot_257")] == [3, 64, 256, 257]


@pytest.mark.parametrize("name", lr.SATURATING)
def test_saturating_cases_hold_every_special_logit(name):
    case, lam, r, s = _ref(name)
    assert all((case["out"]["mdl_outs"] == v).any() for v in lr.SPECIALS)
    assert s["n_pos"] > 0 and math.isfinite(r["loss"])
    sc = case["out"]["mdl_outs"].shape[-1] * lam / r["n_mean"]
    g, x = r["grad_mdl_outs"], case["out"]["mdl_outs"]
    big = r["in_mean"] & (np.abs(x) >= 88)
    sat = np.where(x > 0, 1.0, 0.0) - r["targets"]    # sigmoid saturated: 0 or -+1 times the scale
    if case["conc"] == "sep":
        sat = sat * case["inp"]["num_cmp_msk"][:, :, None, None]
    assert big.sum() >= 4 and np.abs(g[big] - (sat * sc)[big]).max() <= 1e-30


@pytest.mark.parametrize("name", lr.EMPTY + ("noverb_sep",))
def test_empty_mean_cases(name):
    case, lam, r, _ = _ref(name)
    if name == "noverb_sep":
        assert math.isnan(r["verb_loss"]) and r["n_verb"] == 0 and not r["grad_vidf_outs"].any() and math.isfinite(r["loss"])
    else:
        assert math.isnan(r["loss"]) and r["masked"] and r["n_mean"] == 0 and not r["grad_mdl_outs"].any()
