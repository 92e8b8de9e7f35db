"""Inputs, float64 reference and device call for the operator tests of csrc/loss.hip (vog_loss_fwd / vog_loss_bwd).

`make_case` builds the loss-side batch of one geometry directly as numpy from a seed (no model, no forward); the branches the
loss goldens never reach are asked for by name (`edges`, `abm`, `cmp_msk`, `verb`, `logits`). `ref64` is
oracle.vog_oracle.loss_forward on float64 copies, differentiated by torch autograd; `run_device` is the C ABI through lib.py on
guarded buffers. tests/test_loss_edge_host.py pins the oracle against the reference LossB_* on these inputs (fixtures from
oracle/make_golden_loss.py) and asserts that each case reaches the branch it is named for (`stats`); tests/test_gpu_loss_ops.py
compares the kernels with `ref64`.

Boxes. Every coordinate is an integer below 4096, except two edge boxes whose far x is a half integer (below): all widths,
heights, areas and intersections are then exact in fp32 however the compiler contracts `ax*ay + gx*gy - iw*ih`, only the
division rounds, and the quotient nearest to 1/2 without being 1/2 is 1/(2 * union) away (unions stay below 3700, so more
than 1.3e-4). 100/200 is exactly 0.5.

Edge content (`edges=True`), per query, in the rows of the target video and again in one other video (where the target has
to be 0). Proposals, each under the four mask combinations frm only / pnt only / both / neither:
    P0 [0,0,9,9]            10 x 10
    P1 [30,30,30,30]        empty (w = h = 1): IoU -1
    P2 [0,0,0,0]            empty, the all-zero padding row
    P3 [50,60,50.5,60]      1.5 x 1: the only kind of proposal a 1 x 1 gt box can cover by more than half
ground truth (the last 8 slots of the gt block):
    e0 [0,0,9,19]  IoU(P0) = 100/200 exactly      e1 [0,0,9,18]  100/190          e2 [0,5,9,14]  50/150
    e3 [0,0,0,0]   empty, the all-zero padding    e4 [50,60,50,60] empty, away from the origin; IoU(P3) would be 1/1.5
    e5 [0,0,9,9]   = P0                           e6 [30,30,30,30] empty, = P1
    e7 [30,30,30.5,30]  1.5 x 1 round P1: IoU would be 1/1.5 if the empty proposal were not -1
and five argument patterns (gt slots, srl_boxes_lens) cycled over the arguments:
    A (e0,e2,e3 | 1,1,1)  P0 -> 0: only the exact 1/2 is near           B (e1,e2,e3 | 1,1,1)  P0 -> 1: just above
    C (e1,e0,e2 | 0,1,1)  P0 -> 0: the only box above 1/2 has lens 0    D (e3,e4,e6 | 1,1,1)  empty gt only; P3 -> 0 by that rule
    E (e7,e5,e3 | 1,1,1)  P1 -> 0 by the empty-proposal rule, P0 -> 1
Mask bytes are 0 / 1 as the loader hands them over (the reference multiplies by the byte, the device tests `!= 0`)."""
import ctypes as C
import contextlib
import importlib
import types

import numpy as np
import torch

from oracle import vog_oracle as vo

F64 = torch.float64
PROPS = np.array([[0, 0, 9, 9], [30, 30, 30, 30], [0, 0, 0, 0], [50, 60, 50.5, 60]], np.float32)
EDGE_GT = np.array([[0, 0, 9, 19], [0, 0, 9, 18], [0, 5, 9, 14], [0, 0, 0, 0], [50, 60, 50, 60], [0, 0, 9, 9],
                    [30, 30, 30, 30], [30, 30, 30.5, 30]], np.float32)
PATTERNS = (((0, 2, 3), (1, 1, 1)), ((1, 2, 3), (1, 1, 1)), ((1, 0, 2), (0, 1, 1)), ((3, 4, 6), (1, 1, 1)),
            ((7, 5, 3), (1, 1, 1)))
N_EDGE_ROWS = 4 * len(PROPS)
SPECIALS = np.array([0.0, 1e-40, -1e-40, 30.0, -30.0, 88.0, -88.0, 1e4, -1e4], np.float32)


def row_video(conc, ncmp, nfrm, nppf0):
    """video slot of every row of a temp / spat proposal block"""
    r = np.arange(ncmp * nfrm * nppf0)
    return r // (nfrm * nppf0) if conc == "temp" else (r // nppf0) % ncmp


def _logits(rng, shape, kind):
    z = rng.standard_normal(shape)                    # drawn for every kind: the rest of a case does not depend on it
    if kind == "zero":
        return np.zeros(shape, np.float32)
    if kind == "normal":
        return (2.0 * z).astype(np.float32)
    assert kind == "sat", kind
    x = (3.0 * z).astype(np.float32)
    n = x.size
    pick = np.arange(n) % 2 == 0                      # every other element, every special value from 18 elements on
    x.reshape(-1)[pick] = SPECIALS[(np.arange(n)[pick] // 2 * 4 + 3) % len(SPECIALS)]
    return x


def make_case(conc, B, ncmp, nfrm, nppf0, nsrl, nbox, G, nv, seed, *, edges=False, logits="normal", abm="random",
              cmp_msk="ones", verb="random"):
    """-> {'conc', 'nppf0', 'nfrm', 'out': {mdl_outs[, vidf_outs]}, 'inp': {the loss-side batch keys}} as numpy.
    edges: the edge proposals / gt boxes / argument patterns of the module docstring (needs ncmp >= 2, nfrm * nppf0 >= 16,
    G >= 9, nbox >= 3). logits: 'normal' N(0, 2) | 'zero' | 'sat' (0, +-1e-40, +-30, +-88, +-1e4 mixed with N(0, 3)).
    abm (srl_arg_boxes_mask): 'random' | 'zero' | 'last' (only the last entry is 1). cmp_msk (num_cmp_msk): 'ones' | 'some' |
    'zero'. verb (sep; verb_cross_cmp_msk): 'random' | 'none' | 'tail' (only the rows from 256 on, through the last column)."""
    assert conc in ("temp", "spat", "sep")
    sep = conc == "sep"
    assert nv == 1 or (sep and nv == ncmp)
    rng = np.random.default_rng(seed)
    NPv = nfrm * nppf0
    NP = NPv if sep else ncmp * NPv
    lead = (B, ncmp) if sep else (B,)
    target = rng.integers(0, ncmp, B).astype(np.int64)
    # proposals: integer boxes of 13..43 pixels a side, each within 3 pixels of one of three anchor boxes of its block, so that
    # a fair share of the (proposal, gt copy) pairs lies above 1/2; columns 4..6 (frame, score, class) play no part
    which = rng.integers(0, 3, lead + (NP, 1))
    xy = np.take_along_axis(rng.integers(0, 60, lead + (3, 2)), which, -2) + rng.integers(-3, 4, lead + (NP, 2))
    wh = np.take_along_axis(rng.integers(16, 41, lead + (3, 2)), which, -2) + rng.integers(-3, 4, lead + (NP, 2))
    xy = np.maximum(xy, 0)
    props = np.concatenate([xy, xy + wh - 1, rng.integers(0, nfrm, lead + (NP, 1)), rng.random(lead + (NP, 2))],
                           -1).astype(np.float32)
    # ground truth: jittered copies of proposals, random boxes, all-zero padding - all of them reachable by srl_boxes
    gts = np.zeros(lead + (G, 5), np.float32)
    n_cp, n_rd = max(1, G // 3), max(1, G // 3)
    src = rng.integers(0, NP, lead + (n_cp,))
    gts[..., :n_cp, :] = np.take_along_axis(props[..., :5], src[..., None], -2)
    gts[..., :n_cp, :4] += rng.integers(-1, 2, lead + (n_cp, 4))
    rxy, rwh = rng.integers(0, 60, lead + (n_rd, 2)), rng.integers(4, 41, lead + (n_rd, 2))
    gts[..., n_cp:n_cp + n_rd, :4] = np.concatenate([rxy, rxy + rwh - 1], -1)
    frm = (rng.random(lead + (NP, G)) < 0.7).astype(np.uint8)
    pnt = (rng.random(lead + (NP,)) < 0.3).astype(np.uint8)
    srl_boxes = rng.integers(0, G, (B, nv, nsrl, nbox)).astype(np.int64)
    lens = (rng.random((B, nv, nsrl, nbox)) < 0.8).astype(np.int64)
    if abm == "random":
        abm_a = (rng.random((B, nv, nsrl)) < 0.7).astype(np.int64)
        abm_a[0, 0, 0] = 1
    else:
        abm_a = np.zeros((B, nv, nsrl), np.int64)
        if abm == "last":
            abm_a[-1, -1, -1] = 1
        else:
            assert abm == "zero", abm
    if cmp_msk == "ones":
        cm = np.ones((B, ncmp), np.int64)
    elif cmp_msk == "some":
        cm = (rng.random((B, ncmp)) < 0.6).astype(np.int64)
        cm[np.arange(B), target] = 1
        cm[np.arange(B), (target + 1) % ncmp] = 0
        assert ncmp > 1
    else:
        assert cmp_msk == "zero", cmp_msk
        cm = np.zeros((B, ncmp), np.int64)
    if edges:
        assert ncmp >= 2 and NPv >= N_EDGE_ROWS and G >= len(EDGE_GT) + 1 and nbox >= 3
        g0 = G - len(EDGE_GT)
        vid = None if sep else row_video(conc, ncmp, nfrm, nppf0)
        for b in range(B):
            for v in (int(target[b]), int(target[b] + 1) % ncmp):
                blk = (b, v) if sep else (b,)
                gts[blk][g0:, :4] = EDGE_GT
                rows = (np.arange(NPv) if sep else np.nonzero(vid == v)[0])[-N_EDGE_ROWS:]
                for j, box in enumerate(PROPS):
                    for m in range(4):
                        r = rows[4 * j + m]
                        props[blk][r, :4] = box
                        frm[blk][r, g0:] = m & 1
                        pnt[blk][r] = (m >> 1) & 1
        for n in range(B * nv * nsrl):
            if n % 6 == 5:
                continue                                   # every sixth argument keeps its random boxes
            idx, ln = PATTERNS[(n - n // 6) % len(PATTERNS)]
            b, lv, a = n // (nv * nsrl), (n // nsrl) % nv, n % nsrl
            srl_boxes[b, lv, a, :3] = g0 + np.array(idx)
            srl_boxes[b, lv, a, 3:] = g0 + 3
            lens[b, lv, a, :3] = ln
            if abm == "random":
                abm_a[b, lv, a] = 1
    inp = {"pad_proposals": props, "pad_gt_bboxs": gts, "pad_frm_mask": frm, "pad_pnt_mask": pnt, "srl_boxes": srl_boxes,
           "srl_boxes_lens": lens, "srl_arg_boxes_mask": abm_a, "target_cmp": target, "num_cmp_msk": cm,
           "new_srl_idxs": np.zeros((B, ncmp), np.int64)}
    out = {"mdl_outs": _logits(rng, (B, ncmp if sep else 1, nsrl, NP), logits)}
    if sep:
        out["vidf_outs"] = _logits(rng, (B, ncmp), logits)
        inp["verb_cmp"] = rng.integers(0, 2, (B, ncmp)).astype(np.int64)
        if verb == "random":
            vm = (rng.random((B, ncmp, ncmp)) < 0.4).astype(np.int64)
            vm[0, 0, 0] = 1
        else:
            vm = np.zeros((B, ncmp, ncmp), np.int64)
            if verb == "tail":
                assert B * ncmp > 256
                vm.reshape(B * ncmp, ncmp)[256:, -1] = 1
            else:
                assert verb == "none", verb
        inp["verb_cross_cmp_msk"] = vm
    return {"conc": conc, "nppf0": nppf0, "nfrm": nfrm, "out": out, "inp": inp}


# name -> ((conc, B, ncmp, nfrm, nppf0, nsrl, nbox, G, nv, seed), edge arguments, loss_lambda). NP is 3 to 40 and B 1 to 4
# except where a strided loop of loss_finish_kernel needs more than 256 of something.
CASES = {
    # threshold and box conventions; parameters: lambda 0.3, sep with nv == ncmp and with nv == 1 < ncmp
    "thr_spat": (("spat", 2, 2, 2, 10, 5, 3, 12, 1, 11), dict(edges=True), 1.0),
    "thr_temp": (("temp", 2, 2, 2, 10, 5, 4, 12, 1, 12), dict(edges=True), 0.3),
    "thr_sep": (("sep", 2, 2, 2, 10, 6, 3, 12, 2, 13), dict(edges=True), 1.0),
    "thr_sep_nv1": (("sep", 3, 3, 2, 8, 4, 3, 10, 1, 14), dict(edges=True, cmp_msk="some"), 0.3),
    # no argument has boxes: the plain mean over everything
    "plain_temp": (("temp", 2, 2, 2, 5, 3, 2, 6, 1, 21), dict(abm="zero", cmp_msk="some"), 1.0),
    "plain_spat": (("spat", 2, 2, 2, 5, 3, 2, 6, 1, 22), dict(abm="zero", cmp_msk="some"), 1.0),
    "plain_sep": (("sep", 2, 3, 1, 7, 3, 2, 6, 3, 23), dict(abm="zero", cmp_msk="some"), 1.0),
    # strided loops: 313 partial blocks; 260 srl_arg_boxes_mask entries, the last one set; 260 verb rows, the tail unmasked
    "stride_spat_313": (("spat", 4, 4, 10, 100, 5, 3, 12, 1, 31), dict(edges=True, cmp_msk="some"), 1.0),
    "stride_abm_260": (("sep", 13, 4, 1, 3, 5, 2, 5, 4, 32), dict(abm="last", cmp_msk="some"), 1.0),
    "stride_verb_260": (("sep", 65, 4, 1, 3, 1, 2, 5, 1, 33), dict(verb="tail"), 1.0),
    "tot_3": (("temp", 1, 1, 1, 3, 1, 2, 4, 1, 34), {}, 1.0),
    "tot_64": (("spat", 1, 2, 2, 4, 4, 2, 5, 1, 35), {}, 1.0),
    "tot_256": (("temp", 2, 2, 2, 8, 4, 2, 5, 1, 36), {}, 1.0),
    "tot_257": (("spat", 1, 1, 1, 257, 1, 2, 5, 1, 37), {}, 1.0),
    # saturating logits
    "sat_temp": (("temp", 2, 2, 2, 6, 3, 3, 8, 1, 41), dict(logits="sat"), 1.0),
    "sat_sep": (("sep", 3, 3, 1, 8, 2, 3, 8, 3, 42), dict(logits="sat"), 0.3),
    # empty means
    "empty_temp": (("temp", 2, 2, 2, 5, 3, 2, 6, 1, 51), dict(cmp_msk="zero"), 1.0),
    "empty_spat": (("spat", 2, 2, 2, 5, 3, 2, 6, 1, 52), dict(cmp_msk="zero"), 1.0),
    "empty_sep": (("sep", 2, 2, 1, 7, 3, 2, 6, 2, 53), dict(cmp_msk="zero"), 1.0),
    "noverb_sep": (("sep", 2, 2, 1, 7, 3, 2, 6, 2, 54), dict(verb="none"), 1.0),
}
THRESHOLD = ("thr_spat", "thr_temp", "thr_sep", "thr_sep_nv1", "stride_spat_313")
PLAIN = ("plain_temp", "plain_spat", "plain_sep")
SATURATING = ("sat_temp", "sat_sep")
EMPTY = ("empty_temp", "empty_spat", "empty_sep")


def build(name, **override):
    """-> (case, loss_lambda) of CASES[name]; override: edge arguments to replace (logits='zero' for the target map)."""
    args, edge, lam = CASES[name]
    return make_case(*args, **{**edge, **override}), lam


def digest_of(case):
    from oracle import cases
    return cases.digest({**case["inp"], **{"out_" + k: v for k, v in case["out"].items()}})


def oracle_cfg(case):
    return types.SimpleNamespace(conc_type=case["conc"], nppf0=case["nppf0"])


def oracle32(case, loss_lambda=1.0):
    """the fp32 CPU oracle on the case -> {'loss', 'mdl_out_loss'[, 'verb_loss']} as floats"""
    res = vo.loss_forward(oracle_cfg(case), vo.to_torch(case["out"]), vo.to_torch(case["inp"]), loss_lambda)
    return {k: float(v) for k, v in res.items()}


def ref64(case, loss_lambda=1.0):
    """oracle.vog_oracle.loss_forward on float64 copies -> loss values (floats), 'grad_mdl_outs' = d loss / d mdl_outs and
    (sep) 'grad_vidf_outs' = d verb_loss / d vidf_outs (float64 numpy, torch.autograd.grad), 'targets' (bool), 'in_mean'
    (bool: the elements the mean is taken over), 'n_mean', 'masked', 'n_verb', and the two candidate means 'mean_plain' /
    'mean_masked' of the per-element loss (the one the `masked` flag does not choose is what a wrong choice would report)."""
    inp = vo.to_torch(case["inp"])
    inp = {k: v.to(F64) if v.dtype == torch.float32 else v for k, v in inp.items()}
    out = {k: torch.from_numpy(v).to(F64).requires_grad_(True) for k, v in case["out"].items()}
    res = vo.loss_forward(oracle_cfg(case), out, inp, loss_lambda, detail=True)
    r = {k: float(v.detach()) for k, v in res.items() if not k.startswith("_")}
    r["grad_mdl_outs"] = torch.autograd.grad(res["loss"], out["mdl_outs"], retain_graph=True)[0].numpy()
    if "verb_loss" in res:
        r["grad_vidf_outs"] = torch.autograd.grad(res["verb_loss"], out["vidf_outs"])[0].numpy()
        r["n_verb"] = int((res["_vm"] != 0).sum())
    tot, bm = res["_tot"].detach(), res["_bm"]
    r["targets"] = res["_targets"].numpy()
    r["masked"] = res["_masked"]
    r["in_mean"] = (bm != 0).numpy() if r["masked"] else np.ones(tuple(tot.shape), bool)
    r["n_mean"] = int(r["in_mean"].sum())
    r["mean_plain"] = float(tot.mean())
    r["mean_masked"] = float(tot[bm != 0].mean()) if bool((bm != 0).any()) else float("nan")
    return r


# ---- what a case reaches (float64 numpy, written out a second time so that single rules can be left out) -----------------
def gathered(case, empty_gt_rule=True, empty_prop_rule=True):
    """-> (tg [B, nvo, nsrl, NP, nbox]: the gathered IoUs after mask, target-video and lens factors, float64;
    info: 'on' [B, nvo, 1, NP, 1] target-video rows, 'unmasked' / 'egt' (gathered gt box is empty) / 'eprop' like tg)."""
    inp, sep = case["inp"], case["conc"] == "sep"
    P, Gt = inp["pad_proposals"].astype(np.float64), inp["pad_gt_bboxs"].astype(np.float64)
    fm, pm = inp["pad_frm_mask"], inp["pad_pnt_mask"]
    B, ncmp = inp["num_cmp_msk"].shape
    if not sep:
        P, Gt, fm, pm = P[:, None], Gt[:, None], fm[:, None], pm[:, None]
    ax, ay = P[..., 2] - P[..., 0] + 1, P[..., 3] - P[..., 1] + 1
    gx, gy = Gt[..., 2] - Gt[..., 0] + 1, Gt[..., 3] - Gt[..., 1] + 1
    iw = np.clip(np.minimum(P[..., :, None, 2], Gt[..., None, :, 2]) - np.maximum(P[..., :, None, 0], Gt[..., None, :, 0]) + 1, 0, None)
    ih = np.clip(np.minimum(P[..., :, None, 3], Gt[..., None, :, 3]) - np.maximum(P[..., :, None, 1], Gt[..., None, :, 1]) + 1, 0, None)
    ov = iw * ih / ((ax * ay)[..., :, None] + (gx * gy)[..., None, :] - iw * ih)
    unm = np.broadcast_to(((fm | pm[..., None]) != 0), ov.shape)
    egt = np.broadcast_to(((gx == 1) & (gy == 1))[..., None, :], ov.shape)
    epr = np.broadcast_to(((ax == 1) & (ay == 1))[..., :, None], ov.shape)
    ov = ov * unm
    if empty_gt_rule:
        ov = np.where(egt, 0.0, ov)
    if empty_prop_rule:
        ov = np.where(epr, -1.0, ov)
    NP = P.shape[2]
    if sep:
        on = np.arange(ncmp)[None, :, None] == inp["target_cmp"][:, None, None]
        on = np.broadcast_to(on, (B, ncmp, NP))
    else:
        on = (row_video(case["conc"], ncmp, case["nfrm"], case["nppf0"])[None, :] == inp["target_cmp"][:, None])[:, None]
    ov = ov * on[..., None]
    sb, ln = inp["srl_boxes"], inp["srl_boxes_lens"]
    nvo = ncmp if sep else 1
    nsrl, nbox = sb.shape[2:]
    sb, ln = np.broadcast_to(sb, (B, nvo, nsrl, nbox)), np.broadcast_to(ln, (B, nvo, nsrl, nbox))
    shp = (B, nvo, nsrl, NP)
    idx = np.broadcast_to(sb[:, :, :, None, :], shp + (nbox,))

    def take(a):
        return np.take_along_axis(np.broadcast_to(a[:, :, None], shp + (a.shape[-1],)), idx, -1)
    tg = take(ov) * ln[:, :, :, None, :]
    info = {"on": on[:, :, None, :, None], "unmasked": take(unm), "egt": take(egt), "eprop": take(epr),
            "lens": np.broadcast_to(ln[:, :, :, None, :], tg.shape)}
    return tg, info


def stats(case, ref=None):
    """Counts over the elements in the mean, for the conditions of tests/test_loss_edge_host.py."""
    ref = ref or ref64(case)
    tg, info = gathered(case)
    best = tg.max(-1)
    inm = ref["in_mean"]
    assert np.array_equal(best > 0.5, ref["targets"]), "the numpy restatement and the oracle disagree on a target"
    live = inm[..., None] & info["on"] & info["unmasked"] & (info["lens"] != 0)         # gathered IoUs that can decide
    real = live & ~info["egt"] & ~info["eprop"]
    t_gt = gathered(case, empty_gt_rule=False)[0].max(-1) > 0.5
    t_pr = gathered(case, empty_prop_rule=False)[0].max(-1) > 0.5
    inp = case["inp"]
    P = inp["pad_proposals"]
    eprop_rows = (P[..., 2] - P[..., 0] == 0) & (P[..., 3] - P[..., 1] == 0)
    on_rows = info["on"][:, :, 0, :, 0] if case["conc"] == "sep" else info["on"][:, 0, 0, :, 0]
    return {"n_mean": int(inm.sum()), "n_pos": int((ref["targets"] & inm).sum()),
            "gathered_empty_gt": int((live & info["egt"] & ~info["eprop"]).sum()),
            "empty_props_on_target": int((eprop_rows & on_rows).sum()),
            "gathered_empty_prop": int((live & info["eprop"]).sum()),
            "flip_exact_half": int((((best >= 0.5) != (best > 0.5)) & inm).sum()),
            "just_above": int(((best > 0.5) & (best < 0.53) & inm).sum()),
            "flip_without_empty_gt_rule": int(((t_gt != ref["targets"]) & inm).sum()),
            "flip_without_empty_prop_rule": int(((t_pr != ref["targets"]) & inm).sum()),
            "exact_half": int((real & (tg == 0.5)).sum()),
            "near_half": int((real & (tg != 0.5) & (np.abs(tg - 0.5) < 1e-4)).sum())}


# ---- the device ------------------------------------------------------------------------------------------------------------
def loss_args(L, case, dev, loss_lambda):
    """-> (LossArgs with every input pointer and dimension set - out / scratch left NULL -, the device tensors by key)"""
    inp, sep = case["inp"], case["conc"] == "sep"
    t = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in {**case["out"], **inp}.items()}
    a = L.LossArgs()
    for k in ("mdl_outs", "pad_proposals", "pad_gt_bboxs", "pad_frm_mask", "pad_pnt_mask", "srl_boxes", "srl_boxes_lens",
              "srl_arg_boxes_mask", "target_cmp", "num_cmp_msk") + (("vidf_outs", "verb_cmp", "verb_cross_cmp_msk") if sep else ()):
        setattr(a, k, L.ptr(t[k]))
    B, nvo, nsrl, NP = case["out"]["mdl_outs"].shape
    a.B, a.ncmp, a.nv, a.nsrl = B, inp["num_cmp_msk"].shape[1], inp["srl_boxes"].shape[1], nsrl
    a.nbox, a.NP, a.G, a.nppf0 = inp["srl_boxes"].shape[3], NP, inp["pad_gt_bboxs"].shape[-2], case["nppf0"]
    a.conc_type, a.loss_lambda = L.CONC_TYPE[case["conc"]], loss_lambda
    return a, t


def run_device(case, loss_lambda=1.0):
    """vog_loss_fwd then vog_loss_bwd through lib.py on guarded buffers: `out` (6 floats), a scratch of exactly
    vog_loss_scratch_bytes and both gradients each sit between two pattern-filled bands that are checked on exit.
    -> {'out' (after the forward), 'out_after_bwd', 'grad_mdl_outs'[, 'grad_vidf_outs'], 'inputs_after': the device copies of
    every input read back behind the backward} as numpy."""
    from tests.test_gpu_train_ops import guarded
    L = importlib.import_module("vognet-pytorch_amd.lib")
    lib = L.load()
    sep = case["conc"] == "sep"
    a, t = loss_args(L, case, "cuda", loss_lambda)
    nb = int(lib.vog_loss_scratch_bytes(C.byref(a)))
    n_out, n_v = case["out"]["mdl_outs"].size, (case["out"]["vidf_outs"].size if sep else 0)
    assert nb == (n_out + 255) // 256 * 12, nb
    with contextlib.ExitStack() as st:
        res = st.enter_context(guarded(24)).view(torch.float32)
        scr = st.enter_context(guarded(nb))
        g = st.enter_context(guarded(4 * n_out)).view(torch.float32)
        gv = st.enter_context(guarded(4 * n_v)).view(torch.float32) if sep else None
        a.out, a.scratch = L.ptr(res), L.ptr(scr)
        L.check(lib.vog_loss_fwd(C.byref(a), L.stream_ptr()), "vog_loss_fwd")
        torch.cuda.synchronize()
        r = {"out": res.cpu().numpy().copy()}
        L.check(lib.vog_loss_bwd(C.byref(a), L.ptr(g), L.ptr(gv), L.stream_ptr()), "vog_loss_bwd")
        torch.cuda.synchronize()
        r["out_after_bwd"] = res.cpu().numpy().copy()
        r["grad_mdl_outs"] = g.cpu().numpy().reshape(case["out"]["mdl_outs"].shape).copy()
        if sep:
            r["grad_vidf_outs"] = gv.cpu().numpy().reshape(case["out"]["vidf_outs"].shape).copy()
        r["inputs_after"] = {k: v.cpu().numpy() for k, v in t.items()}
    return r
