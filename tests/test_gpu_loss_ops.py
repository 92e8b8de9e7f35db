"""Operator tests of the device loss (csrc/loss.hip: vog_loss_fwd, vog_loss_bwd) through the C ABI, at the branches the loss
goldens never reach: tests/loss_ref.py builds the inputs, tests/test_loss_edge_host.py shows that each case reaches its branch
and that the oracle agrees with the reference LossB_* there, and here the kernels are held to a float64 run of that oracle
(`ref64`). `out`, a scratch of exactly vog_loss_scratch_bytes and both gradients sit between guard bands (`run_device`).

Bounds, the project's own from the golden tests: loss values 2e-5 relative, gradients 1e-6 + 2e-5 max|ref|, the zeros of the
reference gradient exactly zero, out[3..5] exactly the oracle's counts. The fp32 CPU oracle stays inside them against float64
on every case, the saturating ones included (measured worst over all cases: loss 1.8e-7 relative, gradient 8.1e-8 absolute
at a bound of 2.1e-5; sat_temp 1.1e-7 / 1.6e-8, sat_sep 1.7e-7 / 2.2e-9), so no case needs a bound of its own."""
import ctypes as C
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from tests import loss_ref as lr

pytestmark = pytest.mark.gpu
LOSS_TOL = 2e-5


def grad_bound(ref):
    return 1e-6 + 2e-5 * float(np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _run(name, logits=None):
    """(case, lambda, float64 reference, device results), computed once and shared (read-only)"""
    case, lam = lr.build(name, **({"logits": logits} if logits else {}))
    return case, lam, lr.ref64(case, lam), lr.run_device(case, lam)


def _same_value(got, ref, what):
    if math.isnan(ref):
        assert math.isnan(got), (what, got)
        return
    err = abs(got - ref) / max(abs(ref), 1e-30)
    print(f"    {what}: {got!r} vs {ref!r}: {err:.3e} (bound {LOSS_TOL:.0e})")
    assert math.isfinite(got) and err <= LOSS_TOL, (what, got, ref, err)


def _same_grad(got, ref, what):
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err, bound = float(np.abs(got - ref).max()), grad_bound(ref)
    print(f"    {what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)
    assert not got[ref == 0].any(), f"{what}: nonzero where the reference gradient is exactly 0"


@pytest.mark.parametrize("name", list(lr.CASES))
def test_loss_and_gradient_vs_float64(name):
    case, lam, ref, dev = _run(name)
    sep, out = case["conc"] == "sep", dev["out"]
    _same_value(float(out[0]), ref["loss"], "loss")
    _same_value(float(out[1]), ref["mdl_out_loss"], "mdl_out_loss")
    if sep:
        _same_value(float(out[2]), ref["verb_loss"], "verb_loss")
    else:
        assert out[2] == 0
    # the counts the backward divides by, and the choice of the mean
    assert out[3] == ref["n_mean"] and out[4] == float(ref["masked"]) and out[5] == (ref["n_verb"] if sep else 0), out
    _same_grad(dev["grad_mdl_outs"], ref["grad_mdl_outs"], "d loss / d mdl_outs")
    if sep:
        _same_grad(dev["grad_vidf_outs"], ref["grad_vidf_outs"], "d verb_loss / d vidf_outs")
    # the backward writes nothing but the gradients
    assert dev["out_after_bwd"].tobytes() == out.tobytes()
    for k, v in dev["inputs_after"].items():
        src = case["out"][k] if k in case["out"] else case["inp"][k]
        assert v.dtype == src.dtype and v.tobytes() == src.tobytes(), k


@pytest.mark.parametrize("name", lr.PLAIN)
def test_plain_mean(name):
    case, lam, ref, dev = _run(name)
    out, g = dev["out"], dev["grad_mdl_outs"]
    assert out[4] == 0 and out[3] == g.size
    cm = case["inp"]["num_cmp_msk"]
    if case["conc"] == "sep":                  # every element is in the mean, scaled by the video mask
        assert (g[cm != 0] != 0).all() and not g[cm == 0].any()
    else:                                      # the elements a masked mean would leave out (bm == 0: all of them) get gradient
        assert (g != 0).all()


@pytest.mark.parametrize("name", lr.EMPTY + ("noverb_sep",))
def test_empty_means(name):
    case, lam, ref, dev = _run(name)
    out = dev["out"]
    if name == "noverb_sep":
        assert math.isnan(out[2]) and out[5] == 0 and not dev["grad_vidf_outs"].any() and math.isfinite(out[0])
    else:
        assert math.isnan(out[0]) and math.isnan(out[1]) and out[3] == 0 and out[4] == 1 and not dev["grad_mdl_outs"].any()


@pytest.mark.parametrize("name", lr.THRESHOLD + ("tot_256", "tot_257", "plain_temp", "plain_sep"))
def test_target_map_from_zero_logits(name):
    """With all-zero logits the gradient is (1/2 - target) * scale [* video mask]: the device's own target map, element by
    element, against the oracle's on everything in the mean."""
    case, lam, ref, dev = _run(name, "zero")
    g, out = dev["grad_mdl_outs"].astype(np.float64), dev["out"]
    scale = case["out"]["mdl_outs"].shape[-1] * lam / float(out[3])
    inm = ref["in_mean"]
    if case["conc"] == "sep":
        inm = inm & (case["inp"]["num_cmp_msk"] != 0)[:, :, None, None]
    assert inm.sum() > 0 and 0 < (ref["targets"] & inm).sum() < inm.sum()
    assert np.abs(np.abs(g[inm]) - 0.5 * scale).max() <= 1e-6 * scale
    tgt = g < 0
    bad = np.argwhere((tgt != ref["targets"]) & inm)
    assert bad.size == 0, f"{len(bad)} targets differ, first at (b, v, arg, row) = {bad[0]}"


@pytest.mark.parametrize("name", lr.SATURATING)
def test_saturating_logits(name):
    """loss and gradient finite; where |x| >= 88 the gradient is exactly 0 or -+scale [* video mask]"""
    case, lam, ref, dev = _run(name)
    assert np.isfinite(dev["out"]).all()
    x, g = case["out"]["mdl_outs"], dev["grad_mdl_outs"]
    scale = np.float32(x.shape[-1] * lam) / dev["out"][3]
    big = ref["in_mean"] & (np.abs(x) >= 88)
    want = (np.where(x > 0, 1.0, 0.0) - ref["targets"]) * scale
    if case["conc"] == "sep":
        want = want * case["inp"]["num_cmp_msk"][:, :, None, None]
    assert big.sum() >= 4 and np.abs(g[big] - want[big]).max() <= 1e-6 * scale
    huge = ref["in_mean"] & (np.abs(x) >= 1e4)       # exp(-|x|) is 0 in fp32 and in float64: 0 is exactly 0 there
    assert huge.sum() >= 2 and ((g[huge] == 0) == (want[huge] == 0)).all() and (want[huge] == 0).any()


@pytest.mark.parametrize("name", ["thr_sep", "stride_spat_313", "tot_257", "sat_temp"])
def test_two_calls_are_bit_equal(name):
    case, lam, ref, dev = _run(name)
    again = lr.run_device(case, lam)
    for k in ("out", "grad_mdl_outs", "grad_vidf_outs"):
        if k in dev:
            assert again[k].tobytes() == dev[k].tobytes(), k


# ---- argument checks: only descriptors the entries must refuse; nothing is launched, no address is formed -------------------
L = importlib.import_module("vognet-pytorch_amd.lib")
FWD_PTRS = ("mdl_outs", "pad_proposals", "pad_gt_bboxs", "pad_frm_mask", "pad_pnt_mask", "srl_boxes", "srl_boxes_lens",
            "srl_arg_boxes_mask", "target_cmp", "num_cmp_msk", "out", "scratch")
BAD = [("spat", {k: None}) for k in FWD_PTRS] + [
    ("spat", {"nv": 2}), ("spat", {"ncmp": 3}), ("temp", {"ncmp": 3}), ("sep", {"verb_cmp": None}),
    ("sep", {"verb_cross_cmp_msk": None}), ("sep", {"nv": 3}), ("spat", {"B": 0}), ("sep", {"nbox": 0})]


def _valid(conc):
    """a valid descriptor (tot_64 for spat / temp geometry, thr_sep for sep: ncmp 2) with NaN canaries in out and gradients"""
    case, lam = lr.build({"spat": "tot_64", "temp": "tot_256", "sep": "thr_sep"}[conc])
    a, t = lr.loss_args(L, case, "cuda", lam)
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")
    t["out"], t["g"], t["gv"] = nan(6), nan(case["out"]["mdl_outs"].size), nan(case["inp"]["num_cmp_msk"].size)
    t["scratch"] = torch.zeros(int(L.load().vog_loss_scratch_bytes(C.byref(a))), dtype=torch.uint8, device="cuda")
    a.out, a.scratch = L.ptr(t["out"]), L.ptr(t["scratch"])
    return a, t


def _refused(rc, t):
    msg = L.load().vog_last_error()
    torch.cuda.synchronize()
    assert rc != 0 and msg and b"bad argument" in msg, (rc, msg)
    for k in ("out", "g", "gv"):
        assert torch.isnan(t[k]).all(), f"{k} was written by a refused call"


@pytest.mark.parametrize("conc,change", BAD, ids=[f"{c}-{k}={v}" for c, d in BAD for k, v in d.items()])
def test_forward_refuses(conc, change):
    a, t = _valid(conc)
    for k, v in change.items():
        setattr(a, k, v)
    _refused(L.load().vog_loss_fwd(C.byref(a), L.stream_ptr()), t)


@pytest.mark.parametrize("conc,change", [b for b in BAD if "scratch" not in b[1]] + [("spat", {"g": None}), ("spat", {"gv": 1}),
                                                                                     ("sep", {"gv": 1, "vidf_outs": None})],
                         ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else v)
def test_backward_refuses(conc, change):
    """also: no grad_mdl_outs, and grad_vidf_outs given for a loss that is not sep or has no vidf_outs"""
    a, t = _valid(conc)
    g, gv = L.ptr(t["g"]), (L.ptr(t["gv"]) if conc == "sep" else None)
    for k, v in change.items():
        if k == "g":
            g = None
        elif k == "gv":
            gv = L.ptr(t["gv"])
        else:
            setattr(a, k, v)
    _refused(L.load().vog_loss_bwd(C.byref(a), g, gv, L.stream_ptr()), t)


def test_valid_descriptor_of_the_argument_checks_is_accepted():
    for conc in ("spat", "temp", "sep"):
        a, t = _valid(conc)
        L.check(L.load().vog_loss_fwd(C.byref(a), L.stream_ptr()), "vog_loss_fwd")
        L.check(L.load().vog_loss_bwd(C.byref(a), L.ptr(t["g"]), L.ptr(t["gv"]) if conc == "sep" else None, L.stream_ptr()),
                "vog_loss_bwd")
        torch.cuda.synchronize()
        assert torch.isfinite(t["out"]).all() and torch.isfinite(t["g"]).all()
