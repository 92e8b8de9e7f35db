"""Autograd through the model and the loss: `loss_fn(mdl(batch), batch)['loss'].backward()` fills `p.grad`.

The reference trains with plain autograd (`Learner.train_epoch`, utils/trn_utils.py:485-532; the model wrapped in
DistributedDataParallel, code/main_dist.py:72-85; any optimizer from `opt_fn`). Here the model's forward is one
`torch.autograd.Function` (`_ModelFn`) over the device fp32 path of `train.FP32Trainer`:

    forward:  FP32Trainer.forward (fp32, activations kept) + the heads of precise.PreciseForward.run
    backward: vog_score_eval_bwd_f32 (mdl_outs + mdl_outs_eval) -> visual_backward -> language_backward
              (+ the sep verb head: seg_verb_classf, the segment encoder's and final_hidden's gradients)

reading the module's own parameter storage (an optimizer's in-place update is what the next call sees). Only the
parameters that require grad are the Function's inputs; the weight-gradient GEMMs of the others are skipped (NULL
gradient pointers), and so is every part of the backward that reaches none of them. `mdl.training` selects the
train-mode dropouts (the device's counter-based masks, a fresh seed per call, kept for that call's backward).

The path runs only when grad mode is on and a parameter (or `pad_region_feature` / `seg_feature_for_frms`) requires
grad; the default state and every `torch.no_grad()` forward stay on the inference engine, untouched.

Under `torch.autocast("cuda", dtype=torch.bfloat16 | torch.float16)` the forward runs the mixed-precision step
(`FP32Trainer(amp=...)`: every product with 16-bit operands and fp32 accumulation) and its backward runs in the same mode,
whatever the autocast state is when `backward()` runs. Outputs, parameters and gradients stay fp32; with f16, a
`torch.amp.GradScaler`'s scaled gradients pass through unchanged (non-finite values reach the scaler).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import backward as BW
from . import lib as L
from .engine import model_desc_from_cfg

FEATURE_KEYS = ("pad_region_feature", "seg_feature_for_frms")
# never read by the device forward (the reference builds them, code/mdl_vog.py:171-222, but its forward does not use them)
_UNUSED = ("srl_simple_lin.", "lin_tmp.")


def used_param_names(cfg, comm, names) -> List[str]:
    """The parameters (of `names`, state-dict keys) the forward reads for this cfg - the ones that receive a gradient."""
    d = model_desc_from_cfg(cfg, comm)
    kind = cfg.mdl.name
    sep = cfg.ds.conc_type in ("sep", "svsq")
    has_obj = kind == "vgrnd" or (kind == "vog" and bool(d.obj_to_use))
    has_mul = kind == "vog"
    skip = list(_UNUSED)
    if not sep:
        skip.append("seg_verb_classf.")
    if not has_obj:
        skip += ["obj_txf.", "pe_obj_sub_enc."]
    elif not d.obj_use_rel:
        skip.append("pe_obj_sub_enc.")
    if not has_mul:
        skip += ["mult_txf.", "pe_mul_sub_enc."]
    elif not d.mul_use_rel:
        skip.append("pe_mul_sub_enc.")
    return [n for n in names if not n.startswith(tuple(skip))]


def wants_grad(mdl, inp) -> bool:
    """Does this forward take the autograd path? (grad mode on and a parameter or an input feature requires grad)"""
    if not torch.is_grad_enabled():
        return False
    if any(p.requires_grad for p in mdl._cached_params()):
        return True
    return any(torch.is_tensor(v) and v.requires_grad for v in inp.values())


def _trainer(mdl):
    """The FP32Trainer of the module, its `params` re-pointed at the module's parameter storage on every call."""
    from .extended_config import parse_train_attn, parse_train_gemm_amp, parse_train_lstm, parse_train_lstm_amp, parse_train_qkv
    from .train import FP32Trainer
    tr = getattr(mdl, "_grad_trainer", None)
    if tr is None:
        dev = torch.device("cuda", torch.cuda.current_device())
        tr = FP32Trainer(mdl.cfg, mdl.comm, {}, loss_fn=None, lr=0.0, device=str(dev), share_params=True)
        mdl._grad_trainer = tr
    hip = mdl.cfg.get("hip", None) if hasattr(mdl.cfg, "get") else None
    tr.attn = parse_train_attn(hip)                     # cfg.hip.train_attn: the encoder layers' attention operator
    tr.lstm = parse_train_lstm(hip)                     # cfg.hip.train_lstm: the fp32 BiLSTM recurrence
    tr.lstm_amp = parse_train_lstm_amp(hip)             # cfg.hip.train_lstm_amp: the recurrence under autocast
    tr.gemm_amp = parse_train_gemm_amp(hip)             # cfg.hip.train_gemm_amp: the vector tile products under autocast
    tr.qkv = parse_train_qkv(hip)                       # cfg.hip.train_qkv: the Q / K / V projections of mul_tx's layer 0
    return tr


def _check_inputs(mdl, inp, named) -> Tuple[List[str], List[torch.Tensor]]:
    for k, v in inp.items():
        if torch.is_tensor(v) and v.requires_grad and k not in FEATURE_KEYS:
            raise L.VogError(f"input '{k}' requires grad: only {' / '.join(FEATURE_KEYS)} get a gradient from the model")
    feats = [k for k in FEATURE_KEYS if k in inp and inp[k].requires_grad]       # (a cached form carries no raw features)
    for k in feats:
        t = inp[k]
        if not (t.is_cuda and t.dtype == torch.float32):
            raise L.VogError(f"input '{k}' requires grad: it must be an fp32 tensor on the ROCm device")
    for n, p in named:
        if p.requires_grad and not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise L.VogError(f"parameter '{n}' requires grad: it must be a contiguous fp32 tensor on the ROCm device "
                             f"(it is {p.dtype} on {p.device})")
    return feats, [inp[k] for k in feats]


def grad_forward(mdl, inp: Dict[str, torch.Tensor], T: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The model's forward in the autograd path (AnetBaseMdl.forward when `wants_grad`)."""
    named = list(mdl.named_parameters())
    feats, feat_t = _check_inputs(mdl, inp, named)
    tr = _trainer(mdl)
    dev = tr.dev
    # frozen parameters the forward reads may live anywhere: a device fp32 view of them (a copy only where needed)
    tr.params = {n: (p.detach() if (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous())
                     else p.detach().to(dev, torch.float32).contiguous()) for n, p in named}
    used = set(used_param_names(mdl.cfg, mdl.comm, [n for n, _ in named]))
    train_names = tuple(n for n, p in named if p.requires_grad and n in used)
    pmap = dict(named)
    seed_it = getattr(mdl, "_grad_calls", 0)
    mdl._grad_calls = seed_it + 1
    # cached forms (engine.INPUT_FORMS) under the trainer's rule: a batch may carry one once every parameter of the stage it
    # caches has requires_grad = False - `for p in mdl.lstm_encoder.parameters(): p.requires_grad_(False)` and so on
    frozen = frozenset(n for n, p in named if not p.requires_grad)
    vals = _ModelFn.apply(mdl, tr, inp, T, bool(mdl.training), seed_it, tuple(feats), train_names, frozen, *feat_t,
                          *(pmap[n] for n in train_names))
    return dict(zip(_out_keys(mdl.cfg), vals))


def _out_keys(cfg):
    sep = ["vidf_outs", "fin_scores_loss", "fin_scores"] if cfg.ds.conc_type in ("sep", "svsq") else []
    return ["mdl_outs", "mdl_outs_eval"] + sep + ["_pred_rec"]


_AUTOCAST_AMP = {torch.bfloat16: "bf16", torch.float16: "f16"}


def autocast_mode() -> Optional[str]:
    """The precision mode of a forward issued now: None outside autocast, 'bf16' / 'f16' inside torch.autocast("cuda")."""
    if not torch.is_autocast_enabled("cuda"):
        return None
    dt = torch.get_autocast_dtype("cuda")
    if dt not in _AUTOCAST_AMP:
        raise L.VogError(f"torch.autocast('cuda', dtype={dt}): the training path has bf16 and f16 modes only")
    return _AUTOCAST_AMP[dt]


def next_dropout_seed(mdl) -> int:
    """The dropout seed the next autograd forward of `mdl` uses in train mode (csrc/train_dev.h::drop_scale; restated by
    oracle.drop_mask)."""
    return (getattr(mdl, "_grad_calls", 0) + 1) & 0x7FFFFFFFFFFFFFFF


class _ModelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mdl, tr, inp, T, training, seed_it, feats, train_names, frozen, *tensors):
        lib = tr.lib
        d = tr.desc
        tr.dropout, tr.dropout_seed, tr.num_it = training, 0, seed_it        # seed = num_it + 1 (FP32Trainer._step_seed)
        ctx.amp = autocast_mode()                        # (kept: the backward runs in the forward's mode)
        with tr.precision(ctx.amp):
            return _ModelFn._forward(ctx, tr, inp, T, lib, d, feats, train_names, frozen)

    @staticmethod
    def _forward(ctx, tr, inp, T, lib, d, feats, train_names, frozen):
        o, acts, g = tr._forward(inp, T=T, frozen=frozen)
        sep = tr.cfg.ds.conc_type in ("sep", "svsq")
        st = L.stream_ptr()
        B, nc_v, nsrl = g["B"], g["nc_v"], g["nsrl"]
        NP = g["nfrm"] * g["nppf"]
        ncmp = inp["num_cmp_msk"].shape[1]
        nvl = inp["srl_arg_inds_msk"].shape[1]
        logits = o["mdl_outs"]
        arg_msk = inp["srl_arg_inds_msk"].contiguous()
        cmp_msk = inp["num_cmp_msk"].contiguous()
        one = torch.ones(1, dtype=torch.float32, device=tr.dev)
        zero = torch.zeros(1, dtype=torch.float32, device=tr.dev)
        # the heads of the no-grad fp32 forward (precise.PreciseForward.run)
        outs_eval = torch.empty_like(logits)
        outs_copy = torch.empty_like(logits)
        a = L.ScoreArgs()
        a.h1, a.w2, a.b2 = L.ptr(logits), L.ptr(one), L.ptr(zero)
        a.arg_msk, a.cmp_msk = L.ptr(arg_msk), L.ptr(cmp_msk)
        a.outs, a.outs_eval = L.ptr(outs_copy), L.ptr(outs_eval)
        a.n_vid, a.nfrm, a.nppf, a.nsrl, a.dh = B * nc_v, 1, NP, nsrl, 1
        a.conc_type, a.ncmp, a.nc_v, a.nvl = d.conc_type, ncmp, nc_v, nvl
        a.nfrm0, a.nppf0 = d.nfrm0, d.nppf0
        L.check(lib.vog_score_head(C.byref(a), st), "vog_score_head")
        res = {"mdl_outs": logits, "mdl_outs_eval": outs_eval}
        fin = None
        if sep:
            p = tr.params
            v = inp["verb_ind_in_srl"]
            if v.shape[1] == 1 and ncmp > 1:
                v = v.expand(-1, ncmp)
            v = v.contiguous()
            hid = acts["hid"].contiguous()
            ps = acts["obj_x"]
            if ps is None:
                # cached obj_tx rows: there is no [prop | seg] matrix; the head reads its segment block only, rebuilt here
                se = acts["se"]
                zp = torch.zeros(B * nc_v * NP, d.prop_enc, dtype=torch.float32, device=tr.dev)
                ps = torch.empty(B * nc_v * NP, d.prop_enc + se.shape[1], dtype=torch.float32, device=tr.dev)
                L.check(lib.vog_concat_rows_f32(L.ptr(zp), d.prop_enc, 1, L.ptr(se), se.shape[1], d.nppf0, L.ptr(ps), B * nc_v * NP, st),
                        "vog_concat_rows_f32")
            vid_scratch = torch.empty(B, ncmp, dtype=torch.float32, device=tr.dev)
            fin = (torch.empty(B, ncmp, nsrl, dtype=torch.float32, device=tr.dev), torch.empty(B, ncmp, dtype=torch.float32, device=tr.dev))
            pc = L.PredcmpArgs()
            pc.final_hidden, pc.prop_seg = L.ptr(hid), L.ptr(ps)
            pc.w0, pc.b0 = L.ptr(p["seg_verb_classf.0.weight"]), L.ptr(p["seg_verb_classf.0.bias"])
            pc.w2, pc.b2 = L.ptr(p["seg_verb_classf.2.weight"]), L.ptr(p["seg_verb_classf.2.bias"])
            pc.outs, pc.arg_msk, pc.cmp_msk, pc.verb_ind = L.ptr(outs_copy), L.ptr(arg_msk), L.ptr(cmp_msk), L.ptr(v)
            pc.vidf_outs, pc.fin_scores_loss, pc.fin_scores = L.ptr(vid_scratch), L.ptr(fin[0]), L.ptr(fin[1])
            pc.B, pc.ncmp, pc.nvl, pc.nsrl, pc.NP = B, ncmp, nvl, nsrl, NP
            pc.nfrm0, pc.nppf0, pc.L = d.nfrm0, d.nppf0, hid.shape[1]
            pc.dp0, pc.dps = d.prop_enc, ps.shape[1]
            L.check(lib.vog_pred_cmp_head(C.byref(pc), st), "vog_pred_cmp_head")
            res["vidf_outs"] = o["vidf_outs"].clone()              # (a view of the verb head's [B*nc_v, 1] output)
            res["fin_scores_loss"], res["fin_scores"] = fin
            acts["_keep_heads"] = (v, hid, vid_scratch)
        rb = int(lib.vog_pred_record_bytes(ncmp, nsrl, d.nfrm0))
        rec = torch.empty(B, rb // 4, dtype=torch.float32, device=tr.dev)
        pa = L.PredArgs()
        props = inp["pad_proposals"].contiguous()
        pa.outs_eval, pa.props = L.ptr(outs_eval), L.ptr(props)
        pa.fin_scores = L.ptr(fin[1]) if sep else None
        pa.rec = L.ptr(rec)
        pa.B, pa.ncmp, pa.nsrl, pa.nfrm0, pa.nppf0, pa.conc_type = B, ncmp, nsrl, d.nfrm0, d.nppf0, d.conc_type
        L.check(lib.vog_pred_head(C.byref(pa), st), "vog_pred_head")
        res["_pred_rec"] = rec
        ctx.tr, ctx.acts, ctx.g, ctx.inp = tr, acts, g, inp
        ctx.params = dict(tr.params)                     # (the views of this call: a later forward re-points tr.params)
        ctx.feats, ctx.train_names, ctx.sep = feats, train_names, sep
        ctx.masks = (arg_msk, cmp_msk, ncmp, nvl)
        ctx.keep = (one, zero, outs_copy, props, v if sep else None)
        ctx.save_for_backward(logits)
        nd = [res["_pred_rec"]] + ([res["fin_scores_loss"], res["fin_scores"]] if sep else [])
        ctx.mark_non_differentiable(*nd)
        ctx.set_materialize_grads(False)
        ctx.keys = _out_keys(tr.cfg)
        assert set(ctx.keys) == set(res)
        return tuple(res[k] for k in ctx.keys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        with ctx.tr.precision(ctx.amp):
            return _ModelFn._backward(ctx, *grads)

    @staticmethod
    def _backward(ctx, *grads):
        gd = dict(zip(ctx.keys, grads))
        tr, acts, g, inp = ctx.tr, ctx.acts, ctx.g, ctx.inp
        (logits,) = ctx.saved_tensors
        lib, d, p = tr.lib, tr.desc, ctx.params
        need = set(ctx.train_names)
        feat_dx = tuple(k in ctx.feats for k in FEATURE_KEYS)
        st = L.stream_ptr()
        B, nc_v, nsrl = g["B"], g["nc_v"], g["nsrl"]
        NP = g["nfrm"] * g["nppf"]
        arg_msk, cmp_msk, ncmp, nvl = ctx.masks
        d_mo, d_ev, d_vf = gd.get("mdl_outs"), gd.get("mdl_outs_eval"), gd.get("vidf_outs")
        grads: Dict[str, torch.Tensor] = {}
        keep = []
        main = d_mo is not None or d_ev is not None
        if d_ev is not None:
            d_mo = d_mo.contiguous() if d_mo is not None else None
            d_ev = d_ev.contiguous()
            d_logits = torch.empty_like(logits)
            L.check(lib.vog_score_eval_bwd_f32(L.ptr(logits), L.ptr(d_mo), L.ptr(d_ev), L.ptr(arg_msk), L.ptr(cmp_msk), L.ptr(d_logits),
                                               B * nc_v, nsrl, NP, d.conc_type, ncmp, nc_v, nvl, d.nfrm0, d.nppf0, st),
                    "vog_score_eval_bwd_f32")
            keep += [d_mo, d_ev]
        elif d_mo is not None:
            d_logits = d_mo.contiguous()
        else:
            d_logits = torch.zeros_like(logits)
        # the sep verb head: vidf_outs = seg_verb_classf([hid | mean_F(seg_enc)]) (code/mdl_conc_sep.py:64-129)
        d_hid, d_seg_mean = None, None
        if d_vf is not None and ctx.sep:
            sv, h1 = acts["verb_sv"], acts["verb_h1"]
            BV = sv.shape[0]
            w0, b0 = p["seg_verb_classf.0.weight"], p["seg_verb_classf.0.bias"]
            w2, b2 = p["seg_verb_classf.2.weight"], p["seg_verb_classf.2.bias"]
            dvf = d_vf.to(torch.float32).reshape(BV, 1).contiguous()
            r2 = BW.linear_f32(h1, w2, b2, False, dy=dvf, want_dx=True, want_w="seg_verb_classf.2.weight" in need,
                               want_b="seg_verb_classf.2.bias" in need)
            r0 = BW.linear_f32(sv, w0, b0, True, dy=r2["d_x"], want_dx=True, want_w="seg_verb_classf.0.weight" in need,
                               want_b="seg_verb_classf.0.bias" in need)
            for nm, r, k in (("seg_verb_classf.2.weight", r2, "g_w"), ("seg_verb_classf.2.bias", r2, "g_b"),
                             ("seg_verb_classf.0.weight", r0, "g_w"), ("seg_verb_classf.0.bias", r0, "g_b")):
                if r.get(k) is not None:
                    grads[nm] = r[k]
            d_sv = r0["d_x"]                                       # [BV, D + seg_enc]
            Dh = acts["hid"].shape[1]
            rep = 1 if nvl == nc_v else nc_v                       # hid shared by the videos of a query (nv = 1, ncmp > 1)
            d_hid = torch.empty(d_sv.shape[0] // rep, Dh, dtype=torch.float32, device=d_sv.device)
            L.check(lib.vog_rep_sum_f32(L.ptr(d_sv), d_sv.shape[1], rep, None, 0, 1, L.ptr(d_hid), d_hid.shape[0], Dh, st),
                    "vog_rep_sum_f32")
            d_seg_mean = (d_sv, Dh)
            keep += [dvf, r2, r0, d_sv]
        lang_names = [n for n in need if n.startswith(("lstm_encoder.", "lstm_out_feat_proj.", "srl_arg_words_out_enc."))]
        want_lang = bool(lang_names)
        vis_need = set(need) if main else {n for n in need if n.startswith(("seg_encoder.",))}
        if not main:
            # only the verb head's gradient arrived: the segment encoder is reached through the mean alone
            d_logits = torch.zeros_like(logits)
        vg = BW.visual_backward(p, g, acts, d_logits, need=vis_need, want_lang=want_lang and main, d_seg_mean=d_seg_mean,
                                feat_dx=feat_dx if main else (False, feat_dx[1]))
        grads.update({k: v for k, v in vg.items() if not k.startswith("_")})
        if want_lang and (main or d_hid is not None):
            d_lang = vg.get("_d_lang")
            if d_lang is None:                                 # (verb gradient only: nothing reaches the argument vectors)
                w = inp["srl_arg_words_ind"]
                d_lang = torch.zeros(w.shape[0] * w.shape[1] * w.shape[2], p["srl_arg_words_out_enc.0.weight"].shape[0],
                                     dtype=torch.float32, device=logits.device)
            lg = BW.language_backward(p, inp, acts["T"], d.rnn_layers, d_lang_enc=d_lang, drop=g.get("drop_lang"),
                                      forward_scratch=acts["lang_scratch"], need=set(lang_names), d_hid=d_hid)
            for k, v in lg.items():
                if not k.startswith("_") and (main or not k.startswith("srl_arg_words_out_enc.")):
                    grads[k] = v
            keep.append(lg)
        out = [None] * 9
        for k in FEATURE_KEYS:
            if k in ctx.feats:
                dx = vg.get("_d_prop_feat" if k == "pad_region_feature" else "_d_seg_feat")
                out.append(None if dx is None else dx.reshape(inp[k].shape))
        out += [grads.get(n) for n in ctx.train_names]
        ctx.keep_bwd = keep
        return tuple(out)


class _LossFn(torch.autograd.Function):
    """loss_fn's forward with a grad_fn (mdl_conc._LossB.forward when the model's outputs require grad)."""

    @staticmethod
    def forward(ctx, loss_fn, inp, mdl_outs, vidf_outs):
        d = loss_fn._forward_values({"mdl_outs": mdl_outs.detach(), **({"vidf_outs": vidf_outs.detach()} if vidf_outs is not None else {})},
                                    inp)
        ctx.loss_fn, ctx.ld = loss_fn, d
        ctx.has_v = vidf_outs is not None
        ctx.v_shape = vidf_outs.shape if vidf_outs is not None else None
        ctx.set_materialize_grads(False)
        ctx.keys = list(d.keys())
        return tuple(d[k].clone() for k in ctx.keys)            # (d's values are views of one result vector)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        gd = dict(zip(ctx.keys, grads))
        g_loss = [gd[k] for k in ("loss", "mdl_out_loss") if gd.get(k) is not None]   # (the two are the same value)
        g_verb = gd.get("verb_loss")
        want_v = ctx.has_v and g_verb is not None
        d_mo = d_vf = None
        if g_loss or want_v:
            r = ctx.loss_fn.backward(ctx.ld, with_verb=want_v)
            gm, gv = r if want_v else (r, None)
            if g_loss:
                s = g_loss[0] if len(g_loss) == 1 else g_loss[0] + g_loss[1]
                d_mo = gm * s
            if want_v:
                d_vf = gv.reshape(-1) * g_verb
        return None, None, d_mo, (d_vf.reshape(ctx.v_shape) if d_vf is not None else None)
