"""the training step of the reference's `Learner.train_epoch` (utils/trn_utils.py:485-532) for the
VOGNet model on the device:

    out = mdl(batch); loss = loss_fn(out, batch); loss.backward(); optimizer.step()

as forward (fp32, activations kept at the seams) -> `LossB_*` (vog_loss_fwd) -> `LossB_*.backward` (vog_loss_bwd) ->
`visual_backward` + `language_backward` (csrc/train_tx.hip, csrc/train_lang.hip) -> gradient all-reduce over the ranks
(`dist.all_reduce_grads`, the DistributedDataParallel step of code/main_dist.py:72-85) -> Adam (vog_opt_step_f32: every tensor in
one call, the arithmetic of vog_adam_f32; the reference's `torch.optim.Adam(betas=(0.9, 0.99))`, code/main_dist.py:55) -
optionally with loss scaling, overflow skip and gradient clipping decided on the device. Everything is a C-ABI call into
libvog_hip.so; torch tensors are device containers.

This is the fp32 path that pins the MATH against autograd through the reference (every parameter gradient, three
Adam steps); it shares no kernel with the 16-bit inference forward and is not tuned (one GEMM per BiLSTM time step).
Covers ImgGrnd / VidGrnd / VOGNet with every conc_type. `dropout=True` is the reference's train mode (LSTMEncoder 0.1 / 0.1,
attn_drop on attention probabilities and sub-layer outputs) with masks from a counter-based generator on the device - the
reference's masks come from torch's generator, so a step is statistically, not bitwise, its step; with `dropout=False` a
step equals the reference's with the model in eval mode. For sep / svsq the verb head runs forward only:
the reference's `loss` excludes verb_loss (code/mdl_conc_sep.py:434-436).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from typing import Dict, Optional

import torch

from . import backward as BW
from . import lib as L
from .engine import F32_KEYS, OBJ_MODEL_RULE, TRAIN_STAGES, WORD_KEYS, input_form, model_desc_from_cfg, refuse_cached_forms


# precision modes -> the library's "amp" switch (include/vog_hip.h)
AMP_MODES = {None: 0, "bf16": 1, "f16": 2}
# the encoder layers' attention operator: vog_attn_f32 | vog_attn_fused_f32 | the latter with its pipelined kernels (the library's
# "attn_fused_pipe" switch 0 | 1)
ATTN_MODES = ("materialized", "fused", "fused_pipe")
ATTN_FUSED = ("fused", "fused_pipe")        # the modes that run vog_attn_fused_f32


LSTM_MODES = ("stepwise", "fused")          # the fp32 BiLSTM recurrence of vog_lang_f32: the library's "lstm_fused" switch 0 | 1


LSTM_AMP_MODES = ("tile", "split")          # amp's BiLSTM recurrence of vog_lang_f32: the library's "lstm_amp_split" switch 0 | 1


GEMM_AMP_MODES = ("tile", "pipe")           # amp's vector tile products (gemm_f32_b): the library's "gemm_amp_pipe" switch 0 | 1


# the Q / K / V projections of mul_tx's layer 0: the dense products over every token | the two products over the distinct visual
# rows and the argument vectors (vog_attn_f32_vl / vog_attn_fused_f32_vl)
QKV_MODES = ("dense", "factored")


def parse_train_qkv(qkv) -> str:
    if not isinstance(qkv, str) or qkv not in QKV_MODES:
        raise ValueError(f"qkv = {qkv!r}: one of 'dense', 'factored'")
    return qkv


def parse_train_attn(attn) -> str:
    if attn not in ATTN_MODES:
        raise ValueError(f"attn = {attn!r}: one of 'materialized', 'fused', 'fused_pipe'")
    return attn


def parse_train_lstm(lstm) -> str:
    if lstm not in LSTM_MODES:
        raise ValueError(f"lstm = {lstm!r}: one of 'stepwise', 'fused'")
    return lstm


def parse_train_lstm_amp(lstm_amp) -> str:
    if lstm_amp not in LSTM_AMP_MODES:
        raise ValueError(f"lstm_amp = {lstm_amp!r}: one of 'tile', 'split'")
    return lstm_amp


def parse_train_gemm_amp(gemm_amp) -> str:
    if not isinstance(gemm_amp, str) or gemm_amp not in GEMM_AMP_MODES:
        raise ValueError(f"gemm_amp = {gemm_amp!r}: one of 'tile', 'pipe'")
    return gemm_amp


DYNAMIC_INIT_SCALE = 2.0 ** 16      # torch.amp.GradScaler's init_scale


def parse_loss_scale(loss_scale) -> Optional[float]:
    """None | 'dynamic' | a positive finite number (also as text) -> the initial loss scale (None = no scaling)."""
    if loss_scale is None:
        return None
    if isinstance(loss_scale, str) and loss_scale.strip().lower() == "dynamic":
        return DYNAMIC_INIT_SCALE
    try:
        if isinstance(loss_scale, bool):
            raise ValueError
        s = float(loss_scale)
    except (TypeError, ValueError):
        raise ValueError(f"loss_scale = {loss_scale!r}: None, 'dynamic' or a positive number") from None
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"loss_scale = {loss_scale!r}: None, 'dynamic' or a positive number")
    return s


def parse_clip_norm(clip_norm) -> Optional[float]:
    """None | a positive finite number -> the largest gradient norm a step is applied with (None = no clipping)."""
    if clip_norm is None:
        return None
    if isinstance(clip_norm, (bool, str)) or not isinstance(clip_norm, (int, float)):
        raise ValueError(f"clip_norm = {clip_norm!r}: None or a positive number")
    c = float(clip_norm)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"clip_norm = {clip_norm!r}: None or a positive number")
    return c


def _match(names, spec, what):
    """The parameter names `spec` stands for: the name itself, or every name it is a prefix of."""
    if not isinstance(spec, str):
        raise ValueError(f"{what}: {type(spec).__name__} is neither a parameter name nor a prefix (tensors are matched by "
                         "Learner.fit(params_opt_dict=), which knows the module)")
    hit = [k for k in names if k == spec] or [k for k in names if k.startswith(spec)]
    if not hit:
        raise ValueError(f"{what}: '{spec}' matches no parameter")
    return hit


def expand_freeze(names, freeze):
    """`freeze` (stage names of engine.TRAIN_STAGES and / or parameter names / prefixes; a comma list as text is split) -> the
    frozen parameter names. A stage the model does not have (obj on a model without obj_tx) freezes nothing; a name or prefix
    that matches no parameter is a ValueError."""
    if freeze is None:
        return frozenset()
    if isinstance(freeze, str):
        freeze = [x.strip() for x in freeze.split(",") if x.strip()]
    out = set()
    for f in freeze:
        if f in TRAIN_STAGES:
            out.update(k for k in names if k.startswith(TRAIN_STAGES[f]))
        else:
            out.update(_match(names, f, "freeze"))
    return frozenset(out)


# refused INSIDE a group dict: amsgrad / maximize are trainer-wide (FP32Trainer(amsgrad=, maximize=): one flag word per optimiser
# call), capturable has no meaning here
_UNSUPPORTED_FLAGS = ("amsgrad", "maximize", "capturable")
OPTIMIZERS = ("adam", "adamw")


def parse_optimizer(optimizer, amsgrad=False, maximize=False, accum_steps=1):
    """The trainer-wide optimiser arguments, checked without a device -> (optimizer, amsgrad, maximize, accum_steps)."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer = {optimizer!r}: one of {', '.join(OPTIMIZERS)}")
    for name, val in (("amsgrad", amsgrad), ("maximize", maximize)):
        if not isinstance(val, bool):
            raise ValueError(f"{name} = {val!r}: True or False")
    if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
        raise ValueError(f"accum_steps = {accum_steps!r}: an integer >= 1 (micro-batches per optimiser step)")
    return optimizer, amsgrad, maximize, accum_steps


AVG_MODES = {"ema": L.AVG_EMA, "swa": L.AVG_SWA}


def parse_averaging(avg=None, avg_decay=0.999, avg_warmup=False, avg_start=1, avg_every=1):
    """The weight-averaging arguments, checked without a device -> (avg, decay, warmup, start, every); avg None = off."""
    if avg is not None and avg not in AVG_MODES:
        raise ValueError(f"avg = {avg!r}: None, 'ema' or 'swa'")
    if isinstance(avg_decay, (bool, str)) or not isinstance(avg_decay, (int, float)) or not 0.0 <= float(avg_decay) <= 1.0:
        raise ValueError(f"avg_decay = {avg_decay!r}: a number in [0, 1]")
    if not isinstance(avg_warmup, bool):
        raise ValueError(f"avg_warmup = {avg_warmup!r}: True or False")
    for name, val in (("avg_start", avg_start), ("avg_every", avg_every)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 1:
            raise ValueError(f"{name} = {val!r}: an integer >= 1 (counted in applied optimiser steps)")
    return avg, float(avg_decay), avg_warmup, avg_start, avg_every


def resolve_param_groups(names, param_groups=None, freeze=None, betas=(0.9, 0.99), eps: float = 1e-8):
    """torch.optim's parameter groups over the parameter names `names` (state-dict order) -> (groups, frozen).
    param_groups: None (one implicit group over everything: `groups` is None), or a list of {"params": [names or prefixes],
    "lr": float, "weight_decay": float} (lr: None / absent = the trainer's; weight_decay: 0), or a plain list of names /
    prefixes (one group). What no group lists is frozen, and so is what `freeze` names (`expand_freeze`), also inside a group.
    groups: [{"names": sorted names, "lr": float | None, "weight_decay": float}], without the groups that end up empty;
    frozen: frozenset of names. ValueError (with the offending name): overlapping groups, a name that matches no parameter,
    betas / eps other than the trainer's, a truthy amsgrad / maximize / capturable. Needs no device."""
    names = list(names)
    frozen = set(expand_freeze(names, freeze))
    if param_groups is None:
        return None, frozenset(frozen)
    param_groups = list(param_groups)
    if not all(isinstance(g, dict) for g in param_groups):
        param_groups = [{"params": param_groups}]
    groups, seen = [], {}
    for gi, g in enumerate(param_groups):
        what = f"param_groups[{gi}]"
        if "params" not in g:
            raise ValueError(f"{what}: no 'params'")
        if g.get("betas") is not None and tuple(float(b) for b in g["betas"]) != tuple(float(b) for b in betas):
            raise ValueError(f"{what}: betas = {tuple(g['betas'])}, the trainer's are {tuple(betas)}: betas are shared by all groups")
        if g.get("eps") is not None and float(g["eps"]) != float(eps):
            raise ValueError(f"{what}: eps = {g['eps']}, the trainer's is {eps}: eps is shared by all groups")
        for flag in _UNSUPPORTED_FLAGS:
            if g.get(flag):
                raise ValueError(f"{what}: {flag} = {g[flag]!r} is not a per-group setting (amsgrad / maximize are FP32Trainer "
                                 "arguments and hold for every group)")
        lr = g.get("lr")
        wd = float(g.get("weight_decay") or 0.0)
        if lr is not None and not (math.isfinite(float(lr)) and float(lr) >= 0.0):
            raise ValueError(f"{what}: lr = {lr!r}")
        if not (math.isfinite(wd) and wd >= 0.0):
            raise ValueError(f"{what}: weight_decay = {g.get('weight_decay')!r}")
        specs = [g["params"]] if isinstance(g["params"], str) else list(g["params"])
        mine = []
        for spec in specs:
            for k in _match(names, spec, what):
                if k in seen and seen[k] != gi:
                    raise ValueError(f"{what}: parameter '{k}' is already in param_groups[{seen[k]}]: groups must not overlap")
                if k not in seen:
                    seen[k] = gi
                    mine.append(k)
        mine = sorted(k for k in mine if k not in frozen)
        if mine:
            groups.append({"names": mine, "lr": None if lr is None else float(lr), "weight_decay": wd})
    frozen.update(k for k in names if k not in seen)
    return groups, frozenset(frozen)


class FP32Trainer:
    """`loss_scale` / `clip_norm` (both None by default: the update is plain Adam, one fused call): with either set, the
    optimiser step measures the gradients on the device first (vog_opt_step_f32, mode B) and nothing is read back.
      loss_scale: 'dynamic' (initial scale 2^16, torch.amp.GradScaler's) or a positive number - the initial scale when
        growth_interval > 0, a fixed one when growth_interval == 0. The seed gradient of the backward is multiplied by the
        scale on the device; a step with a non-finite gradient is skipped and the scale multiplied by backoff_factor, and after
        growth_interval clean steps in a row it is multiplied by growth_factor (GradScaler.update). The loss dict `step`
        returns and what `gradients` returns are unscaled.
      clip_norm: the gradients are scaled so that their global L2 norm is at most clip_norm (torch.nn.utils.clip_grad_norm_).
        A clipping-only trainer runs with scale 1 and STILL SKIPS a step whose gradients are not finite - where
        clip_grad_norm_ followed by Adam.step would write the NaN into every parameter. Its scale stays 1 whatever
        growth_interval says: neither clean steps nor a skipped one move it.
    With statistics on, the number of applied steps lives on the device: `scaler_state()` reads the 32-byte state block and
    refreshes `adam_step` (a skipped step does not count).

    Fine-tuning. `freeze`: stage names ('lang', 'enc', 'obj': engine.TRAIN_STAGES) and / or parameter names / prefixes that are
    not trained; `param_groups`: torch.optim's parameter groups by name (`resolve_param_groups`), each with its own lr and L2
    weight_decay - what no group lists is frozen too. A frozen parameter gets no gradient (the backward stops where nothing
    below is trained), takes no part in the all-reduce, the gradient norm or the overflow decision, has no m / v and keeps
    its bits. With both None nothing changes, neither in launches nor in bits.
    Optimiser variants (trainer-wide; with all four at their defaults the step makes the calls it always made):
      optimizer: 'adam' (a group's weight_decay is the L2 form) | 'adamw' (it is decoupled: p *= 1 - lr * weight_decay);
      amsgrad: the denominator uses the running maximum of v (`self.vmax`, saved as `max_exp_avg_sq`); maximize: ascend;
      accum_steps = N: a WINDOW of N calls of `step` makes one update. Every call runs forward, loss and backward (the loss
        scale cannot move inside a window: only the optimiser call moves it); the first call's gradient tensors become the
        accumulators, later calls add into them on the device (vog_opt_accum_f32); only the window's last call exchanges
        gradients across the ranks - once, on the sums (DistributedDataParallel's no_sync pattern) - and runs the optimiser on
        sum / N. `num_it` counts calls (it numbers the dropout masks), `adam_step` counts updates. `flush()` applies a partial
        window (sum / its own count); `gradients()` neither reads nor changes a window.
    Weight averaging (`avg`: None = off, the step makes the calls it always made | 'ema' | 'swa'): behind every optimiser update
      (once per accumulation window, also from `flush`) vog_opt_average_f32 moves `self.avg[k]` towards the updated parameter -
      torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(avg_decay) / get_swa_multi_avg_fn(). Whether an update
      averages is decided on the device from the count of APPLIED steps s (s >= avg_start and (s - avg_start) % avg_every == 0)
      and the optimiser's overflow flag, so a skipped step does not average and nothing is read back; `avg_warmup` caps EMA's
      decay at (1 + n) / (10 + n). A frozen parameter has no average (it is its own); one that becomes trainable later starts
      from a clone of its value. `averaged_state_dict()` is what an evaluation loads; averaging never touches p, m, v or vmax.
    A batch may carry a cached form (engine.INPUT_FORMS) in place of the keys it replaces once EVERY parameter of the stage it
    caches is frozen: the forward then starts behind that stage. Such rows are eval-mode results, so a stage fed in cached
    form has no dropout; a frozen stage fed with raw keys under dropout=True keeps its masks, as a frozen module left in
    train mode does in the reference."""

    def __init__(self, cfg, comm, state_dict: Dict[str, torch.Tensor], loss_fn, lr: Optional[float] = None,
                 betas=(0.9, 0.99), eps: float = 1e-8, device: str = "cuda", process_group=None, dropout: bool = False,
                 dropout_seed: int = 0, bf16_gemm: bool = False, share_params: bool = False, amp: Optional[str] = None,
                 loss_scale=None, clip_norm: Optional[float] = None, growth_interval: int = 2000, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, param_groups=None, freeze=None, optimizer: str = "adam", amsgrad: bool = False,
                 maximize: bool = False, accum_steps: int = 1, avg: Optional[str] = None, avg_decay: float = 0.999,
                 avg_warmup: bool = False, avg_start: int = 1, avg_every: int = 1, attn: str = "materialized",
                 lstm: str = "stepwise", lstm_amp: str = "tile", gemm_amp: str = "tile", qkv: str = "dense"):
        self.optimizer, self.amsgrad, self.maximize, self.accum_steps = parse_optimizer(optimizer, amsgrad, maximize, accum_steps)
        self.avg_mode, self.avg_decay, self.avg_warmup, self.avg_start, self.avg_every = parse_averaging(
            avg, avg_decay, avg_warmup, avg_start, avg_every)
        if amp not in AMP_MODES:
            raise ValueError(f"amp = {amp!r}: one of None, 'bf16', 'f16'")
        # the encoder layers' attention operator: 'materialized' = vog_attn_f32 ([S, N, N] probabilities in scratch, a launch
        # sequence per head) | 'fused' = vog_attn_fused_f32 (csrc/train_attn.hip: O(N) scratch, three launches for all heads;
        # the forward keeps lse beside the concatenated heads) | 'fused_pipe' = the same operator on its pipelined kernels (two
        # LDS buffers, one barrier per staged tile; the bits of 'fused'; a per-thread switch of the library, set in precision()).
        # The default makes the calls it always made.
        self.attn = parse_train_attn(attn)
        # the fp32 BiLSTM recurrence: 'stepwise' = a recurrent product and a cell launch per layer, direction and step | 'fused' =
        # one launch per layer and step for both directions (csrc/train_lang.hip: lstm_ksplit_{fwd,bwd}_kernel<OpF32>). A per-thread
        # switch of the library, set in precision(); amp has fused kernels of its own and ignores it.
        self.lstm = parse_train_lstm(lstm)
        # the BiLSTM recurrence under amp: 'tile' = a workgroup owns 16 units, a wave a whole gate and all of K | 'split' = K split
        # over the waves of a workgroup (csrc/train_lang.hip: lstm_ksplit_{fwd,bwd}_kernel<Op16>; same operands and rounding, another
        # order of the fp32 sums). A per-thread switch of the library, set in precision(); without amp it changes nothing.
        self.lstm_amp = parse_train_lstm_amp(lstm_amp)
        # the vector tile products under amp: 'tile' = the single-buffer 128 x 64 kernel | 'pipe' = the pipelined kernel
        # (csrc/train_gemm.hip: gemm16_pipe_kernel; same operands, rounding and order of the fp32 sums, so the same bits). A
        # per-thread switch of the library, set in precision(); without amp it changes nothing.
        self.gemm_amp = parse_train_gemm_amp(gemm_amp)
        # the Q / K / V projections of mul_tx's layer 0, whose tokens are [obj_tx row of the proposal | masked argument vector]:
        # 'dense' = three [M, d] x [d, d] products over every token, as in every other layer | 'factored' = the products over the
        # distinct visual rows and over the argument vectors, added per token in one launch; the backward sums dQ / dK / dV back to
        # the two factors before its products (csrc/train_tx.hip: vl_*_kernel). Another order of the fp32 sums, not the same bits.
        # mul_x is still built (the layer's residual reads it). No effect on a model without mul_tx.
        self.qkv = parse_train_qkv(qkv)
        if amp is not None and bf16_gemm:
            raise ValueError("amp and bf16_gemm are two precision modes: pass one of them")
        self.loss_scale, self.clip_norm = parse_loss_scale(loss_scale), parse_clip_norm(clip_norm)
        if isinstance(growth_interval, bool) or not isinstance(growth_interval, int) or growth_interval < 0:
            raise ValueError(f"growth_interval = {growth_interval!r}: an integer >= 0 (0 = the scale is fixed)")
        if not (float(growth_factor) >= 1.0 and math.isfinite(float(growth_factor)) and 0.0 < float(backoff_factor) <= 1.0):
            raise ValueError(f"growth_factor = {growth_factor!r} (>= 1), backoff_factor = {backoff_factor!r} (in (0, 1])")
        self.growth_interval, self.growth_factor, self.backoff_factor = growth_interval, float(growth_factor), float(backoff_factor)
        if not torch.cuda.is_available():
            raise RuntimeError("FP32Trainer needs a GPU (libvog_hip.so kernels; there is no CPU fallback)")
        self.lib = L.load()
        self.cfg, self.loss_fn = cfg, loss_fn
        d = model_desc_from_cfg(cfg, comm)
        if cfg.mdl.name not in ("vog", "vgrnd", "igrnd"):
            raise NotImplementedError(f"no device training step for mdl.name = {cfg.mdl.name}")
        self.desc = d
        self.dev = torch.device(device)
        # share_params: the parameters ARE the given tensors (fp32, contiguous, on the device; the caller keeps them there) -
        # the autograd path's forward reads the module's own storage, which an optimizer updates in place (autograd.py)
        self.params = {k: (v.detach() if share_params else v.detach().to(self.dev, torch.float32).contiguous().clone())
                       for k, v in state_dict.items() if torch.is_tensor(v) and v.is_floating_point()}
        self.m: Dict[str, torch.Tensor] = {}
        self.v: Dict[str, torch.Tensor] = {}
        self.vmax: Dict[str, torch.Tensor] = {}                 # (amsgrad only)
        self._acc: Dict[str, torch.Tensor] = {}                 # the open accumulation window: summed gradients, their count
        self._acc_n = 0
        self.avg: Dict[str, torch.Tensor] = {}                  # (avg = 'ema' | 'swa' only) the averaged parameters
        self._avg_state: Optional[torch.Tensor] = None          # their vog_opt_avg_state on the device, made by the first update
        self.lr = float(cfg.train.lr if lr is None else lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self._freeze = freeze
        self._groups, self.frozen = resolve_param_groups(list(self.params), param_groups, freeze, self.betas, self.eps)
        # two counters (round 5): `num_it` = the Learner's iteration count (numbers the dropout masks; restored from a
        # checkpoint on every resume, utils/trn_utils.py:588-590); `adam_step` = torch.optim.Adam's per-parameter `step`
        # (bias correction), which the reference restores ONLY with the optimizer state (`load_opt`, :594-605) - a resume
        # without it builds a fresh Adam at step 0 whose m / v are zero.
        self.num_it = 0
        self.adam_step = 0
        # statistics on (loss_scale or clip_norm): one vog_opt_state on the device - the scale, the growth tracker and the
        # count of APPLIED steps live there, the host's `adam_step` follows it in scaler_state()
        self._opt_state: Optional[torch.Tensor] = None
        self._opt_scratch: Optional[torch.Tensor] = None
        if self.loss_scale is not None or self.clip_norm is not None:
            self._write_opt_state(1.0 if self.loss_scale is None else self.loss_scale, 0, 0)
        self.pg = process_group
        # train-mode dropout (`mdl.train()` in Learner.train_epoch): LSTMEncoder's 0.1 / 0.1 (utils/mdl_srl_utils.py:77), the
        # transformers' cfg.mdl.{obj,mul}_tx.attn_drop on attention probabilities and sub-layer outputs; masks come from a
        # counter-based generator seeded per step (csrc/train_dev.h::drop_scale) - NOT torch's stream, so a step is
        # statistically, not bitwise, the reference's. Off: a step equals the reference's in eval mode.
        # mixed precision: the tile GEMMs round their operands to bf16 (fp32 accumulation, fp32 master weights, fp32 everything
        # else); off = the fp32 path that is pinned against autograd through the reference. A per-thread switch of the library
        # (vog_train_set_int), set at the top of every step.
        self.bf16_gemm = bool(bf16_gemm)
        # amp = 'bf16' | 'f16': autocast's policy - EVERY product of the step (tile, split-K, weight-stream, the fused BiLSTM
        # recurrence) takes 16-bit operands with fp32 accumulation; softmax, LayerNorm, cell nonlinearities, dropout, column
        # sums, the loss and Adam stay fp32, and so do the parameters (master weights) and their gradients
        self.amp = amp
        self.dropout, self.dropout_seed = bool(dropout), int(dropout_seed)
        self.share_params = bool(share_params)
        # the captured step (`capture`): `_layout_epoch` counts what invalidates a slot wholesale (set_param_groups); `_dev` is
        # the slot whose capture is being recorded - its per-step values then come from device memory (the dropout seed's base
        # in place of the seed, the optimiser's device tables)
        self._layout_epoch = 0
        self._dev = None
        self._guard_block: Optional[torch.Tensor] = None        # (the sticky word of `_bounded`'s length guard)
        self.p_lstm = (0.1, 0.1)
        self.p_obj, self.p_mul = float(cfg.mdl.obj_tx.attn_drop), float(cfg.mdl.mul_tx.attn_drop)

    # ---- geometry of one batch (Conc{TEMP,SPAT}: code/mdl_conc_single.py:24-37, 131-143)
    def _geo(self, batch):
        d = self.desc
        B, ncmp = batch["num_cmp_msk"].shape
        nc_v = 1
        if self.cfg.ds.conc_type == "temp":
            nfrm, nppf = ncmp * d.nfrm0, d.nppf0
        elif self.cfg.ds.conc_type == "spat":
            nfrm, nppf = d.nfrm0, ncmp * d.nppf0
        else:                                           # sep / svsq: every video is its own sequence set (mdl_conc_sep.py:14-26)
            nc_v, nfrm, nppf = ncmp, d.nfrm0, d.nppf0
        name = self.cfg.mdl.name                       # ImgGrnd: encoders + lin2; VidGrnd: + obj_tx; VOGNet: + mul_tx (mdl_vog.py:286-744)
        has_obj = name == "vgrnd" or (name == "vog" and d.obj_to_use)
        seed = self._step_seed()
        dr = dict(drop_obj=(self.p_obj, seed), drop_mul=(self.p_mul, seed), drop_lang=self.p_lstm + (seed,)) if self.dropout else {}
        if self.attn in ATTN_FUSED:
            dr["attn_fused"] = True
        return dict(**dr, B=B, nc_v=nc_v, nfrm=nfrm, nppf=nppf, nsrl=d.nsrl, nppf0=d.nppf0, mul_layers=d.mul_layers if name == "vog" else 0,
                    mul_heads=d.mul_heads, mul_use_rel=bool(d.mul_use_rel), obj_layers=d.obj_layers if has_obj else 0, obj_heads=d.obj_heads,
                    obj_use_rel=bool(d.obj_use_rel), obj_one_frm=bool(d.obj_one_frm), vid_w=d.vid_w, vid_h=d.vid_h)

    def _step_seed(self) -> int:
        """One seed per optimisation step (forward and backward of a step recompute the same masks from it)."""
        if self._dev is not None:                               # the base; the kernels add the device's tick (train_dev.h::Drop)
            return step_seed_base(self.dropout_seed)
        return (self.dropout_seed * 1000003 + self.num_it + 1) & 0x7FFFFFFFFFFFFFFF

    def _stack_forward(self, stack, n_layers, pe_name, x, S, N, n, heads, boxes, drop=None, vl=None):
        """-> (output, kept = (layer inputs, concatenated heads) for the backward). vl: layer 0's input as its factors."""
        y, *kept = BW.stack_forward(self.params, stack, n_layers, pe_name, x, S, N, n, heads, boxes, drop=drop,
                                    **({"fused": True} if self.attn in ATTN_FUSED else {}), **({"vl": vl} if vl is not None else {}))
        return y, tuple(kept)

    @contextlib.contextmanager
    def precision(self, amp=None):
        """The library's per-thread precision switches for the calls inside (`amp`: a mode that overrides self.amp), reset to
        off behind them, also when they raise."""
        amp = self.amp if amp is None else amp
        switches = {b"bf16_gemm": 1 if (self.bf16_gemm and amp is None) else 0, b"amp": AMP_MODES[amp],
                    b"lstm_fused": 1 if self.lstm == "fused" else 0, b"lstm_amp_split": 1 if self.lstm_amp == "split" else 0,
                    b"gemm_amp_pipe": 1 if self.gemm_amp == "pipe" else 0, b"attn_fused_pipe": 1 if self.attn == "fused_pipe" else 0}
        for name, value in switches.items():
            L.check(self.lib.vog_train_set_int(name, value), "vog_train_set_int")
        try:
            yield
        finally:
            for name in switches:
                self.lib.vog_train_set_int(name, 0)

    def set_param_groups(self, param_groups) -> None:
        """Replace the parameter groups (`Learner.fit(params_opt_dict=)`); None = every parameter in one group at `self.lr`. The
        constructor's `freeze` stays in force. Moments of parameters that are frozen from now on are dropped (a new
        torch optimizer has no state for parameters it was not given). If a parameter that was frozen becomes trainable, the
        optimiser starts afresh - every moment dropped, the count of applied steps back to 0 - as the reference's `fit` does
        when it builds a new optimizer: the step count is shared by all tensors, and zero moments under an advanced count would
        switch the bias correction off for the newcomer (a first update of about 3.2 x lr). Freezing more, or changing only
        lr / weight_decay, keeps the state of what is still trained."""
        was = self.frozen
        self._layout_epoch += 1                                 # (a captured slot is stale from here on)
        self._groups, self.frozen = resolve_param_groups(list(self.params), param_groups, self._freeze, self.betas, self.eps)
        if any(k not in self.frozen for k in was):
            self.m.clear()
            self.v.clear()
            self.vmax.clear()
            self.adam_step = 0
            if self._opt_state is not None:
                s = self.scaler_state()
                self._write_opt_state(s["scale"], s["growth_tracker"], 0, s["skipped"])
                self.adam_step = 0
        for k in list(self.m):
            if k in self.frozen:
                del self.m[k], self.v[k]
                self.vmax.pop(k, None)
        # averaging: a frozen parameter is its own average; one that joins a running average starts from its value, which is
        # the exact average of what was constant until now
        for k in list(self.avg):
            if k in self.frozen:
                del self.avg[k]
        if self.avg:
            for k in was:
                if k not in self.frozen and k not in self.avg:
                    self.avg[k] = self.params[k].clone()

    def frozen_stages(self):
        """The stages of engine.TRAIN_STAGES the model has and this trainer trains no parameter of."""
        out = []
        for st, pre in TRAIN_STAGES.items():
            mine = [k for k in self.params if k.startswith(pre)]
            if mine and all(k in self.frozen for k in mine):
                out.append(st)
        return out

    def trainable(self, frozen=None):
        """The names whose gradient a step computes: None = all (nothing is frozen)."""
        frozen = self.frozen if frozen is None else frozen
        return {k for k in self.params if k not in frozen} if frozen else None

    def forward(self, batch, T=None):
        """Forward on the device in the trainer's precision mode (see `_forward`)."""
        with self.precision():
            return self._forward(batch, T)

    def check_lengths(self) -> None:
        """For the eager steps run with `T=`: reads the length guard's sticky word (one 16-byte copy) and raises VogError if a
        step had to clamp a sentence length or a capture position to its T - that step trained on a truncated sentence. What
        `TrainSlot.check()` is for a slot. A trainer that never ran a step with `T=` has nothing to check."""
        if self._guard_block is not None and int(self._guard_block.cpu()[3]) != 0:
            raise L.VogError("check_lengths: a step was given a T shorter than a sentence of its batch; the length was clamped and "
                             "that step computed a truncated sentence")

    def _bounded(self, batch, T):
        """The batch as a caller-given sentence bound T may see it: without T (the lengths are read on the host), with a cached
        language form, or inside a capture (the step's tick guards the static tensors in place) the batch itself; otherwise a
        shallow copy whose lengths and capture positions are device copies clamped to T by the tick's guard - a length beyond T
        would index past the T rows the language kernels lay out. The guard's sticky word lands in `self._guard_block`
        (`check_lengths` reads it)."""
        if T is None or self._dev is not None or input_form(batch, WORD_KEYS) is not None:
            return batch
        if self._guard_block is None:
            self._guard_block = torch.zeros(4, dtype=torch.int32, device=self.dev)
        lens = batch["srl_arg_word_mask_len"].to(self.dev, torch.int64).contiguous().clone()
        cap = batch["srl_arg_words_capture"].to(self.dev, torch.int64).contiguous().clone()
        L.check(self.lib.vog_train_tick(L.ptr(self._guard_block), L.ptr(lens), lens.numel(), int(T), None, None, 0, 0, L.TICK_BEGIN, 0,
                                        L.ptr(cap), cap.numel(), L.stream_ptr()), "vog_train_tick")
        return {**batch, "srl_arg_word_mask_len": lens, "srl_arg_words_capture": cap}

    def _rows(self, batch, key, width, rows=None):
        """A cached form's key as fp32 rows [*, width] on the device."""
        t = batch[key]
        if t.shape[-1] != width or (rows is not None and t.numel() != rows * width):
            raise L.VogError(f"'{key}' has shape {tuple(t.shape)}: the model takes {'%d rows of ' % rows if rows is not None else ''}"
                             f"width {width}")
        return t.to(self.dev, torch.float32).reshape(-1, width).contiguous()

    def _forward(self, batch, T=None, frozen=None):
        """fp32 forward on the device -> ({'mdl_outs' [B, nc_v, nsrl, NP] (, 'vidf_outs' [B, ncmp])}, activations at the seams of
        the backward, geometry). `T`: the longest sentence if the caller knows it (a slot does): no host read of the lengths.
        `frozen`: the frozen parameter names if not the trainer's own (the autograd path's: requires_grad). A cached form whose
        stage is frozen is read in place of that stage's result: enc -> the encoder outputs, obj -> obj_tx's output rows (and
        the segment encodings for the sep verb head), vec -> the argument vectors (and the final hidden state for sep / svsq)."""
        frozen = self.frozen if frozen is None else frozen
        refuse_cached_forms(batch, "trainer", frozen=frozen, params=list(self.params))
        feat, lform = input_form(batch, F32_KEYS[:2]), input_form(batch, WORD_KEYS)
        g = self._geo(batch)
        p, lib, st = self.params, self.lib, L.stream_ptr()
        B, nc_v, nfrm, nppf, nsrl = g["B"], g["nc_v"], g["nfrm"], g["nppf"], g["nsrl"]
        NP = nfrm * nppf
        BV = B * nc_v                                                   # model "videos" (sequence sets)
        sep = self.cfg.ds.conc_type in ("sep", "svsq")
        msk = batch["srl_arg_inds_msk"].to(self.dev, torch.int64).contiguous()
        nv = msk.shape[1]
        assert nv in (1, nc_v), "language axis does not match conc_type"
        f32 = lambda k: batch[k].to(self.dev, torch.float32)
        if lform is None:
            T = int(batch["srl_arg_word_mask_len"].max()) if T is None else int(T)
            lf = BW.language_backward(p, batch, T, self.desc.rnn_layers, drop=g.get("drop_lang"))
            lang, hid, lang_scratch = lf["_lang_enc"], lf["_hid"], lf["_scratch"]
        else:                                                           # argument vectors of the frozen language side: no vog_lang_f32, no T
            T, lang_scratch, hid = None, None, None
            lang = self._rows(batch, lform.keys[0], p["srl_arg_words_out_enc.0.weight"].shape[0], B * nv * nsrl)
            if sep:
                if lform.keys[1] not in batch:
                    raise L.VogError(f"a sep / svsq model reads '{lform.keys[1]}' next to '{lform.keys[0]}' (the verb head's feature)")
                hid = self._rows(batch, lform.keys[1], p["lstm_out_feat_proj.0.weight"].shape[0], B * nv)
        props = f32("pad_proposals").reshape(BV * NP, -1).contiguous()
        prop_feat = seg_feat = pe = obj_x = None
        penc, senc = p["prop_encoder.0.weight"].shape[0], p["seg_encoder.0.weight"].shape[0]
        if feat is None:
            prop_feat = f32("pad_region_feature").reshape(BV * NP, -1).contiguous()
            seg_feat = f32("seg_feature_for_frms").reshape(-1, batch["seg_feature_for_frms"].shape[-1]).contiguous()
            pe = BW.linear_f32(prop_feat, p["prop_encoder.0.weight"], p["prop_encoder.0.bias"], True)["y"]
            se = BW.linear_f32(seg_feat, p["seg_encoder.0.weight"], p["seg_encoder.0.bias"], True)["y"]
        else:                                                           # rows of the frozen encoders (and obj_tx): no vog_linear_f32 for them
            se = self._rows(batch, "enc_seg_feature", senc)
            if feat.name == "enc":
                pe = self._rows(batch, feat.keys[0], penc, BV * NP)
        assert se.shape[0] * g["nppf0"] == BV * NP
        if feat is None or feat.name == "enc":
            obj_x = torch.empty(BV * NP, pe.shape[1] + se.shape[1], dtype=torch.float32, device=self.dev)
            L.check(lib.vog_concat_rows_f32(L.ptr(pe), pe.shape[1], 1, L.ptr(se), se.shape[1], g["nppf0"], L.ptr(obj_x), BV * NP, st),
                    "vog_concat_rows_f32")
        obj_out, obj_kept, mul_kept = obj_x, None, None
        if feat is not None and feat.name == "obj":
            if not (sep and g["obj_layers"] > 0):
                raise L.VogError(OBJ_MODEL_RULE)
            obj_out = self._rows(batch, feat.keys[0], penc + senc, BV * NP)
        elif g["obj_layers"] > 0:
            if g["obj_one_frm"]:
                S, N, fdiv = BV * nfrm, nppf, float(nfrm)
            else:
                S, N, fdiv = BV, NP, 1.0
            ob = BW._Boxes(props, g["vid_w"], g["vid_h"], fdiv) if g["obj_use_rel"] else None
            obj_out, obj_kept = self._stack_forward("obj_txf", g["obj_layers"], "pe_obj_sub_enc.0", obj_x, S, N, N, g["obj_heads"], ob,
                                                    drop=g.get("drop_obj"))
        lang_per_vid = 1 if (nv == nc_v and nc_v > 1) else 0
        dobj, dlang = obj_out.shape[1], lang.shape[1]
        # the [vis | lang] tokens: regrouped per frame for mul_tx, in (video, arg, proposal) order when lin2 reads them directly
        hf, hp = (nfrm, nppf) if g["mul_layers"] > 0 else (1, NP)
        mul_x = torch.empty(BV * nfrm * nsrl * nppf, dobj + dlang, dtype=torch.float32, device=self.dev)
        L.check(lib.vog_conc_f32_fwd(L.ptr(obj_out), L.ptr(lang), L.ptr(msk), L.ptr(mul_x), B, nc_v, hf, hp, nsrl, dobj, dlang,
                                     lang_per_vid, st), "vog_conc_f32_fwd")
        y, mul_vl = mul_x, None
        if g["mul_layers"] > 0:
            mb = BW._Boxes(props, g["vid_w"], g["vid_h"], float(nfrm)) if g["mul_use_rel"] else None
            if self.qkv == "factored":                                  # layer 0's attention reads the factors of mul_x
                mul_vl = BW.FactoredInput(obj_out, lang, msk, B, nc_v, nfrm, nppf, nsrl, lang_per_vid=bool(lang_per_vid))
            y, mul_kept = self._stack_forward("mult_txf", g["mul_layers"], "pe_mul_sub_enc.0", mul_x, BV * nfrm, nsrl * nppf, nppf,
                                              g["mul_heads"], mb, drop=g.get("drop_mul"), vl=mul_vl)
        M, dm = y.shape
        dhead = p["lin2.0.weight"].shape[0]
        scratch = torch.empty(M * dhead, dtype=torch.float32, device=self.dev)
        outs = torch.empty(B, nc_v, nsrl, NP, dtype=torch.float32, device=self.dev)
        L.check(lib.vog_score_head_f32(L.ptr(y), L.ptr(p["lin2.0.weight"]), L.ptr(p["lin2.0.bias"]), L.ptr(p["lin2.2.weight"]),
                                       L.ptr(p["lin2.2.bias"]), L.ptr(outs), L.ptr(scratch), scratch.numel() * 4, M, dm, dhead, BV,
                                       hf, hp, nsrl, st), "vog_score_head_f32")
        out = {"mdl_outs": outs}
        if sep:
            # verb head (mdl_conc_sep.py:64-129): reported by LossB_SEP as verb_loss; the reference's `loss` does not include
            # it (`out_loss = mdl_out_loss`, mdl_conc_sep.py:434-436), so nothing flows back through it
            Fv = se.shape[0] // BV                                      # (hid: [B*nv, D])
            seg_mean = torch.empty(BV, se.shape[1], dtype=torch.float32, device=self.dev)
            L.check(lib.vog_row_mean_f32(L.ptr(se), L.ptr(seg_mean), BV, Fv, se.shape[1], st), "vog_row_mean_f32")
            sv = torch.empty(BV, hid.shape[1] + se.shape[1], dtype=torch.float32, device=self.dev)
            L.check(lib.vog_concat_rows_f32(L.ptr(hid), hid.shape[1], 1 if nv == nc_v else nc_v, L.ptr(seg_mean), se.shape[1], 1,
                                            L.ptr(sv), BV, st), "vog_concat_rows_f32")
            h1 = BW.linear_f32(sv, p["seg_verb_classf.0.weight"], p["seg_verb_classf.0.bias"], True)["y"]
            out["vidf_outs"] = BW.linear_f32(h1, p["seg_verb_classf.2.weight"], p["seg_verb_classf.2.bias"], False)["y"].reshape(B, nc_v)
        # kept for the backward: the inputs and concatenated heads of every encoder layer, the language side's whole scratch
        acts = {"mul_x": mul_x, "obj_x": obj_x, "prop_feat": prop_feat, "seg_feat": seg_feat, "props": props, "inds_msk": msk, "T": T,
                "mul_kept": mul_kept, "obj_kept": obj_kept, "lang_scratch": lang_scratch, "hid": hid, "obj_out": obj_out, "lang": lang,
                "se": se}
        if mul_vl is not None:
            acts["mul_vl"] = mul_vl
        if "vidf_outs" in out:                                          # (the verb head's inputs: its backward in autograd.py)
            acts["verb_sv"], acts["verb_h1"] = sv, h1
        return out, acts, g

    def gradients(self, batch, exchange: bool = False, T=None):
        """-> (loss dict, {parameter name: gradient}) of one batch (no update). exchange: average the gradients over the
        ranks - the visual side's buckets are in flight while the language side's backward runs. T: the language kernels'
        sentence bound if the caller knows one (no host read of the lengths; every length must be <= T)."""
        with self.precision():
            ld, grads = self._gradients(batch, exchange, T)
        if self.loss_scale is not None:                         # the contract is the unscaled gradient in every mode (no host read)
            inv = 1.0 / self._opt_state.view(torch.float32)[0]
            grads = {k: v * inv for k, v in grads.items()}
        return ld, grads

    def _gradients(self, batch, exchange, T=None):
        """-> (loss dict, gradients as the optimiser step takes them: multiplied by the loss scale when one is active)."""
        batch = self._bounded(batch, T)
        out, acts, g = self._forward(batch, T)
        ld = self.loss_fn(out, batch)
        d_outs = self.loss_fn.backward(ld)
        if self.loss_scale is not None:                         # the loss values above stay unscaled
            L.check(self.lib.vog_opt_scale_grad_f32(L.ptr(d_outs), d_outs.numel(), L.ptr(self._opt_state), L.stream_ptr()),
                    "vog_opt_scale_grad_f32")
        need = self.trainable()
        if need is None:                                        # nothing frozen: the full backward
            want_lang, vis_kw, lang_kw = True, {}, {}
        else:
            lang_need = {k for k in need if k.startswith(TRAIN_STAGES["lang"])}
            want_lang = bool(lang_need)
            vis_kw, lang_kw = dict(need=need, want_lang=want_lang), dict(need=lang_need)
        grads = BW.visual_backward(self.params, g, acts, d_outs, **vis_kw)
        gv = {k: v for k, v in grads.items() if not k.startswith("_")}
        fin_v = None
        if exchange:
            from .dist import all_reduce_grads_begin
            fin_v = all_reduce_grads_begin(gv)
        gl, fin_l = {}, None
        if want_lang:                                           # (a frozen language side has no backward)
            lg = BW.language_backward(self.params, batch, acts["T"], self.desc.rnn_layers, d_lang_enc=grads["_d_lang"],
                                      drop=g.get("drop_lang"), forward_scratch=acts["lang_scratch"], **lang_kw)
            gl = {k: v for k, v in lg.items() if not k.startswith("_")}
        if exchange:
            if gl:
                fin_l = all_reduce_grads_begin(gl)
            fin_v()
            if fin_l is not None:
                fin_l()
        gv.update(gl)
        return ld, gv

    def _multi(self) -> bool:
        return self.pg is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                       and torch.distributed.get_world_size() > 1)

    def step(self, batch, T=None):
        """One `train_epoch` iteration: forward, loss, backward, (all-reduce,) Adam. -> the loss dict. With accum_steps > 1 the
        gradients join the open window and the window's last call applies it (`flush`). T: the language kernels' sentence bound
        if the caller knows one (a loader does): no host read of the lengths; every length must be <= T."""
        if self.accum_steps == 1:
            with self.precision():
                ld, grads = self._gradients(batch, exchange=self._multi(), T=T)
            self.num_it += 1
            self._optimizer_step(grads)
            return ld
        with self.precision():
            ld, grads = self._gradients(batch, exchange=False, T=T)
        self.num_it += 1
        self._accumulate(grads)
        if self._acc_n >= self.accum_steps:
            self.flush()
        return ld

    def _accumulate(self, grads) -> None:
        """The window's sums: the first call's tensors themselves, `acc += g` in one call afterwards (name order)."""
        if self._acc_n == 0:
            self._acc = {k: v.contiguous() for k, v in grads.items()}
            self._acc_n = 1
            return
        if set(grads) != set(self._acc):
            raise RuntimeError("the trainable parameters changed inside an accumulation window: call flush() first")
        keys = sorted(grads)
        keep = [grads[k].contiguous() for k in keys]
        arr = (L.OptAccumTensor * len(keys))()
        for i, k in enumerate(keys):
            arr[i].acc, arr[i].g, arr[i].n = L.ptr(self._acc[k]), L.ptr(keep[i]), self._acc[k].numel()
        L.check(self.lib.vog_opt_accum_f32(arr, len(keys), L.stream_ptr()), "vog_opt_accum_f32")
        self._acc_n += 1

    def flush(self) -> None:
        """Apply the open window - the sums over its micro-batches, exchanged across the ranks once, times 1 / their count -
        and close it. A no-op on an empty window (also with accum_steps = 1, where no window ever opens)."""
        if self._acc_n == 0:
            return
        grads, n = self._acc, self._acc_n
        self._acc, self._acc_n = {}, 0
        if self._multi():
            from .dist import all_reduce_grads
            all_reduce_grads(grads)
        self._optimizer_step(grads, grad_scale=1.0 / n)

    def set_lr(self, lr, group_lrs=None) -> None:
        """A scheduler's hand on the learning rates: the trainer's own, and every group's (`group_lrs`, one per group in order;
        None = every group takes `lr`). A group without a rate of its own that is given the trainer's keeps following it."""
        lr = float(lr)
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError(f"lr = {lr!r}")
        self.lr = lr
        if self._groups is None:
            return
        if group_lrs is None:
            group_lrs = [lr] * len(self._groups)
        if len(group_lrs) != len(self._groups):
            raise ValueError(f"{len(group_lrs)} learning rates for {len(self._groups)} parameter groups")
        for grp, glr in zip(self._groups, group_lrs):
            if not (math.isfinite(float(glr)) and float(glr) >= 0.0):
                raise ValueError(f"lr = {glr!r}")
            if not (grp["lr"] is None and float(glr) == lr):    # (a group without a rate of its own keeps following the trainer's)
                grp["lr"] = float(glr)

    def group_lrs(self):
        """The learning rate of every parameter group in order (one implicit group without groups)."""
        if self._groups is None:
            return [self.lr]
        return [self.lr if g["lr"] is None else g["lr"] for g in self._groups]

    def _opt_flags(self) -> int:
        return ((L.OPT_DECOUPLED if self.optimizer == "adamw" else 0) | (L.OPT_AMSGRAD if self.amsgrad else 0)
                | (L.OPT_MAXIMIZE if self.maximize else 0))

    def _optimizer_step(self, grads, grad_scale: float = 1.0) -> None:
        """One update: the optimiser call and, with averaging on, the averaging call over the tensors it covered."""
        keys = self._adam_call(grads, grad_scale)
        if self.avg_mode is not None and keys:
            self._average(keys)

    def _average(self, keys) -> None:
        """vog_opt_average_f32 behind the optimiser call, same stream: mode B on the optimiser's device block when there is one
        (its applied-step count and overflow flag decide), mode A with the `adam_step` just counted otherwise."""
        if self._avg_state is None:
            self._avg_state = torch.zeros(4, dtype=torch.int32, device=self.dev)
        arr = (L.OptAvgTensor * len(keys))()
        for i, k in enumerate(keys):
            p = self.params[k]
            if k not in self.avg:
                self.avg[k] = torch.zeros_like(p)               # (the first update overwrites it)
            arr[i].avg, arr[i].p, arr[i].n = L.ptr(self.avg[k]), L.ptr(p), p.numel()
        a = L.OptAvgArgs()
        a.tensors, a.n_tensors = arr, len(keys)
        a.mode, a.decay, a.warmup = AVG_MODES[self.avg_mode], self.avg_decay, int(self.avg_warmup)
        a.start, a.every = self.avg_start, self.avg_every
        if self._opt_state is not None:
            a.opt_state = L.ptr(self._opt_state)
        else:
            a.step = self.adam_step
        a.state = L.ptr(self._avg_state)
        if self._dev is not None:                               # captured: mode A's count is the step block's
            L.check(self.lib.vog_opt_average_dev_f32(ctypes.byref(a), L.ptr(self._dev.block), L.stream_ptr()), "vog_opt_average_dev_f32")
            return
        L.check(self.lib.vog_opt_average_f32(ctypes.byref(a), L.stream_ptr()), "vog_opt_average_f32")

    def avg_state(self) -> dict:
        """{'n_averaged', 'updated', 'w'} after the last update: one 16-byte copy from the device, the host's only read."""
        if self._avg_state is None:
            return {"n_averaged": 0, "updated": 0, "w": 0.0}
        h = L.OptAvgState.from_buffer_copy(self._avg_state.cpu().numpy().tobytes())
        return {"n_averaged": int(h.n_averaged), "updated": int(h.updated), "w": float(h.w)}

    def averaged_state_dict(self) -> Dict[str, torch.Tensor]:
        """Every parameter's average under the reference's key names - the tensors themselves, not copies (hand them to
        `refresh_from_device`, or clone them to keep them). A parameter without an average of its own (frozen, or before any
        update) maps to the parameter itself. Without `avg` this is a ValueError."""
        if self.avg_mode is None:
            raise ValueError("averaged_state_dict: this trainer was built without avg = 'ema' | 'swa'")
        started = self._avg_state is not None and self.avg_state()["n_averaged"] > 0
        return {k: (self.avg[k] if started and k in self.avg else v) for k, v in self.params.items()}

    def averaging_state_dict(self) -> Optional[dict]:
        """What a checkpoint carries of the averaging (None when it is off): the settings, the update count, the averages."""
        if self.avg_mode is None:
            return None
        return {"mode": self.avg_mode, "decay": self.avg_decay, "warmup": self.avg_warmup, "start": self.avg_start,
                "every": self.avg_every, "n_averaged": self.avg_state()["n_averaged"],
                "averaged": {k: v.clone() for k, v in self.avg.items()}}

    def load_averaging_state_dict(self, asd) -> None:
        """Restores what `averaging_state_dict` saved: the averages and their count (the schedule and the decay stay this
        trainer's own). Another mode than this trainer's is a ValueError, as is an average for an unknown or reshaped parameter."""
        if self.avg_mode is None:
            raise ValueError("load_averaging_state_dict: this trainer was built without avg = 'ema' | 'swa'")
        if asd.get("mode") != self.avg_mode:
            raise ValueError(f"averaging state of mode {asd.get('mode')!r} loaded into a trainer with avg = {self.avg_mode!r}")
        new = {}
        for k, v in asd["averaged"].items():
            if k not in self.params:
                raise ValueError(f"averaging state for '{k}', which is no parameter of this model")
            if tuple(v.shape) != tuple(self.params[k].shape):
                raise ValueError(f"averaging state '{k}' has shape {tuple(v.shape)}, the parameter has {tuple(self.params[k].shape)}")
            if k not in self.frozen:
                new[k] = v.to(self.dev, torch.float32).contiguous().clone()
        self.avg = new
        self._write_avg_state(int(asd["n_averaged"]))

    def _write_avg_state(self, n_averaged: int) -> None:
        t = torch.tensor([int(n_averaged), 0, 0, 0], dtype=torch.int32)
        if self._avg_state is None:
            self._avg_state = t.to(self.dev)
        else:
            self._avg_state.copy_(t)

    def _adam_call(self, grads, grad_scale: float = 1.0):
        """Adam over every tensor of `grads` in ONE call, in name order. Without loss scale and clipping:
        mode A, the bits of vog_adam_f32 per tensor, `adam_step` counted here. With either: mode B behind the (already
        exchanged, hence rank-identical) gradients - statistics, decision and update on the stream, no host read; the device
        counts the applied steps. Without parameter groups the call is vog_opt_step_f32 at `self.lr`; with them
        vog_opt_step_groups_f32 over a table ordered group by group (name order inside a group), every group with its own lr
        (None = `self.lr`) and weight decay. `grads` holds trainable tensors only, so frozen ones are in no table.
        With adamw / amsgrad / maximize or a grad_scale other than 1 the call is vog_opt_step_ex_f32 over the same table (one
        implicit group without parameter groups), with `self.vmax` beside m / v under amsgrad."""
        flags = self._opt_flags()
        dev = self._dev                                         # a capture in progress: vog_opt_step_dev_f32 over the same table
        extended = flags != 0 or grad_scale != 1.0 or dev is not None
        keys, spans = self._opt_spans(grads)
        if not keys:
            return keys
        if extended and spans is None:
            spans = [(0, len(keys), self.lr, 0.0)]
        keep = []                                               # (contiguous copies live until the launches are issued)
        arr = (L.OptTensor * len(keys))()
        total = 0
        for i, k in enumerate(keys):
            p = self.params[k]
            if k not in self.m:
                self.m[k], self.v[k] = torch.zeros_like(p), torch.zeros_like(p)
            gk = grads[k].contiguous()
            keep.append(gk)
            t = arr[i]
            t.p, t.g, t.m, t.v, t.n = L.ptr(p), L.ptr(gk), L.ptr(self.m[k]), L.ptr(self.v[k]), p.numel()
            total += p.numel()
        ex = L.OptExArgs()
        ga = ex.groups if extended else L.OptGroupsArgs()
        a = ga.base if spans is not None else L.OptArgs()
        a.tensors, a.n_tensors = arr, len(keys)
        a.lr, a.beta1, a.beta2, a.eps = self.lr, self.betas[0], self.betas[1], self.eps
        if self._opt_state is None and dev is not None:
            pass                                                # (counted in the step block; the host follows per replay)
        elif self._opt_state is None:
            self.adam_step += 1
            a.step = self.adam_step
        else:
            need = int(self.lib.vog_opt_scratch_bytes(len(keys), total))
            if self._opt_scratch is None or self._opt_scratch.numel() < need:
                self._opt_scratch = torch.empty(need, dtype=torch.uint8, device=self.dev)
            a.state, a.scratch, a.scratch_bytes = L.ptr(self._opt_state), L.ptr(self._opt_scratch), self._opt_scratch.numel()
            a.max_norm = 0.0 if self.clip_norm is None else self.clip_norm
            # clipping only: nothing multiplies the gradients by a scale, so the scale stays 1 (interval 0 = it never changes)
            a.growth_factor, a.backoff_factor = self.growth_factor, self.backoff_factor
            a.growth_interval = self.growth_interval if self.loss_scale is not None else 0
        if spans is None:
            L.check(self.lib.vog_opt_step_f32(ctypes.byref(a), L.stream_ptr()), "vog_opt_step_f32")
            return keys
        garr = (L.OptGroup * len(spans))()
        for i, (first, count, lr, wd) in enumerate(spans):
            garr[i].first, garr[i].count, garr[i].lr, garr[i].weight_decay = first, count, lr, wd
        ga.groups, ga.n_groups = garr, len(spans)
        if not extended:
            L.check(self.lib.vog_opt_step_groups_f32(ctypes.byref(ga), L.stream_ptr()), "vog_opt_step_groups_f32")
            return keys
        ex.flags, ex.grad_scale = flags, grad_scale
        if self.amsgrad:
            vm = (ctypes.c_void_p * len(keys))()
            for i, k in enumerate(keys):
                if k not in self.vmax:
                    self.vmax[k] = torch.zeros_like(self.params[k])
                vm[i] = L.ptr(self.vmax[k])
            ex.vmax = vm
        if dev is not None:
            L.check(self.lib.vog_opt_step_dev_f32(ctypes.byref(ex), ctypes.byref(dev.opt_dev_args(len(spans))), L.stream_ptr()),
                    "vog_opt_step_dev_f32")
            return keys
        L.check(self.lib.vog_opt_step_ex_f32(ctypes.byref(ex), L.stream_ptr()), "vog_opt_step_ex_f32")
        return keys

    def _opt_spans(self, names):
        """The optimiser call's table over the tensors `names`: (keys in table order, spans = [(first, count, lr, weight_decay)]
        group by group, or None without parameter groups: one implicit group at `self.lr`)."""
        if self._groups is None:
            return sorted(names), None
        keys, spans = [], []
        for grp in self._groups:
            ks = [k for k in grp["names"] if k in names]
            if ks:
                spans.append((len(keys), len(ks), self.lr if grp["lr"] is None else grp["lr"], grp["weight_decay"]))
                keys += ks
        return keys, spans

    def capture(self, batch, T=None, log_rows: int = 64, keep_graph: bool = False) -> "TrainSlot":
        """The whole iteration on `batch`'s shape - forward, device loss, backward, optimiser, averaging - captured ONCE into a
        graph: `slot.step(batch)` copies a batch into the slot's static tensors and replays it with one launch. Opt-in; `step`
        makes the calls it always made. See `TrainSlot`. Refused (`capture_refusal`): accum_steps > 1, more than one rank, the
        autograd path - those stay eager."""
        why = capture_refusal(self.accum_steps, 2 if self._multi() else 1, "autograd" if self.share_params else "trainer")
        if why:
            raise L.VogError(why)
        return TrainSlot(self, batch, T, log_rows, keep_graph)

    # ---- the device's optimiser state (statistics on)
    def _write_opt_state(self, scale: float, growth_tracker: int, adam_step: int, skipped: int = 0) -> None:
        h = L.OptState(scale=float(scale), growth_tracker=int(growth_tracker), adam_step=int(adam_step), skipped=int(skipped))
        t = torch.frombuffer(bytearray(bytes(h)), dtype=torch.int32)
        if self._opt_state is None:
            self._opt_state = t.to(self.dev)
        else:
            self._opt_state.copy_(t)

    def scaler_state(self) -> dict:
        """{'scale', 'growth_tracker', 'adam_step', 'found_inf', 'grad_norm', 'coef', 'skipped'} after the last step: one
        32-byte copy from the device (this is the host's only read of it), which also refreshes `adam_step`. A trainer
        without loss scale and clipping keeps no statistics: scale 1, nothing skipped, grad_norm None."""
        if self._opt_state is None:
            return {"scale": 1.0, "growth_tracker": 0, "adam_step": self.adam_step, "found_inf": 0, "grad_norm": None, "coef": 1.0,
                    "skipped": 0}
        h = L.OptState.from_buffer_copy(self._opt_state.cpu().numpy().tobytes())
        self.adam_step = int(h.adam_step)
        return {"scale": float(h.scale), "growth_tracker": int(h.growth_tracker), "adam_step": int(h.adam_step),
                "found_inf": int(h.found_inf), "grad_norm": float(h.grad_norm), "coef": float(h.coef), "skipped": int(h.skipped)}

    def scaler_state_dict(self) -> Optional[dict]:
        """torch.amp.GradScaler.state_dict()'s layout; None when no loss scale is active."""
        if self.loss_scale is None:
            return None
        s = self.scaler_state()
        return {"scale": s["scale"], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": s["growth_tracker"]}

    def load_scaler_state_dict(self, ssd) -> None:
        """Restores what `scaler_state_dict` saved (or a GradScaler's state); ignored by a trainer without loss scale."""
        if self.loss_scale is None or not ssd:
            return
        scale = parse_loss_scale(float(ssd["scale"]))
        self.growth_factor, self.backoff_factor = float(ssd["growth_factor"]), float(ssd["backoff_factor"])
        self.growth_interval = int(ssd["growth_interval"])
        s = self.scaler_state()
        self._write_opt_state(scale, int(ssd["_growth_tracker"]), s["adam_step"], s["skipped"])

    def broadcast_from_rank0(self, with_optimizer: bool = False) -> None:
        """What DistributedDataParallel does at construction (code/main_dist.py:72-85): every rank starts from rank 0's
        parameters (and Adam state, after a resume with load_opt) - replicas seeded differently would otherwise apply the
        averaged gradient to different weights. Name order; a no-op without a multi-rank group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1):
            return
        for k in sorted(self.params):
            dist.broadcast(self.params[k], src=0, group=self.pg)
        if with_optimizer:
            for k in sorted(self.params):
                if k not in self.m:
                    self.m[k], self.v[k] = torch.zeros_like(self.params[k]), torch.zeros_like(self.params[k])
                dist.broadcast(self.m[k], src=0, group=self.pg)
                dist.broadcast(self.v[k], src=0, group=self.pg)
                if self.amsgrad:
                    if k not in self.vmax:
                        self.vmax[k] = torch.zeros_like(self.params[k])
                    dist.broadcast(self.vmax[k], src=0, group=self.pg)
            t = torch.tensor([self.num_it, self.adam_step], dtype=torch.int64, device=self.dev)
            dist.broadcast(t, src=0, group=self.pg)
            self.num_it, self.adam_step = int(t[0].item()), int(t[1].item())
            if self._opt_state is not None:                     # scale, tracker and applied steps: rank 0's block
                dist.broadcast(self._opt_state, src=0, group=self.pg)
                self.scaler_state()
            if self.avg_mode is not None:                       # the averages and their count: rank 0's
                if self._avg_state is None:
                    self._write_avg_state(0)
                dist.broadcast(self._avg_state, src=0, group=self.pg)
                # only tensors that HAVE an average (a zero-filled newcomer would pass for one once n_averaged > 0): every
                # rank restored the same checkpoint, so the names agree - checked by their count
                n = torch.tensor([len(self.avg)], dtype=torch.int64, device=self.dev)
                dist.broadcast(n, src=0, group=self.pg)
                if int(n.item()) != len(self.avg):
                    raise RuntimeError(f"rank 0 holds {int(n.item())} averaged tensors, this rank {len(self.avg)}: the ranks did not "
                                       "restore the same averaging state")
                for k in sorted(self.avg):
                    dist.broadcast(self.avg[k], src=0, group=self.pg)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The parameters under the reference's key names (load into the inference model with `load_state_dict`)."""
        return {k: v.clone() for k, v in self.params.items()}

    # ---- checkpoint in the reference's layout (Learner.save_model_dict / load_model_dict, utils/trn_utils.py:533-630)
    def optimizer_state_dict(self):
        """torch.optim.Adam.state_dict() layout (parameters numbered in state-dict key order). `step` is the number of APPLIED
        steps: with statistics on it is read from the device first. Without parameter groups: one group over every position
        (frozen parameters simply have no state)."""
        self.scaler_state()
        keys = list(self.params)
        state = {i: {"step": torch.tensor(float(self.adam_step)), "exp_avg": self.m[k].clone(), "exp_avg_sq": self.v[k].clone()}
                 for i, k in enumerate(keys) if k in self.m}
        if self.amsgrad:                                        # (m / v without vmax: a state loaded or broadcast, not yet stepped)
            for i, k in enumerate(keys):
                if i in state:
                    state[i]["max_exp_avg_sq"] = self.vmax[k].clone() if k in self.vmax else torch.zeros_like(self.v[k])
        # the flags as torch's own Adam / AdamW report them (torch.optim.AdamW is Adam with decoupled_weight_decay = True)
        common = {"betas": self.betas, "eps": self.eps, "amsgrad": self.amsgrad, "maximize": self.maximize}
        if self.optimizer == "adamw":
            common["decoupled_weight_decay"] = True
        if self._groups is None:
            return {"state": state, "param_groups": [{"lr": self.lr, **common, "weight_decay": 0, "params": list(range(len(keys)))}]}
        # with parameter groups: one entry per group; positions still count over the WHOLE model (they stay stable whatever is
        # frozen); frozen parameters are in no group and have no state
        pos = {k: i for i, k in enumerate(keys)}
        return {"state": state,
                "param_groups": [{"lr": self.lr if g["lr"] is None else g["lr"], **common,
                                  "weight_decay": g["weight_decay"], "params": sorted(pos[k] for k in g["names"])}
                                 for g in self._groups]}

    def load_optimizer_state_dict(self, osd):
        """Adam state by POSITION in state-dict key order - torch.optim.Adam numbers `mdl.parameters()`, which for the reference's
        modules is the order of `state_dict()` restricted to parameters. A state whose shape is not its parameter's (a
        checkpoint of another mdl.name / conc_type, or of a model with other sizes) is refused: vog_adam_f32 walks m / v with
        the parameter's element count. Restored: the moments, the step count, betas and eps; lr where the trainer has no
        parameter groups; with groups, every group's lr / weight_decay if the saved groups cover the same positions as this
        trainer's - otherwise they stay this trainer's and a warning says so. A state for a parameter that is frozen now is
        refused. (`Learner` loads a checkpoint before `fit` names its groups: there `fit`'s own lr / groups apply.)"""
        keys = list(self.params)
        new_m, new_v, new_x, adam_step = {}, {}, {}, self.adam_step
        for i, stt in osd["state"].items():
            if not 0 <= int(i) < len(keys):
                raise ValueError(f"optimizer state for parameter #{i}, the model has {len(keys)}")
            k = keys[int(i)]
            if k in self.frozen:
                raise ValueError(f"optimizer state for parameter #{i} ({k}), which is frozen now: a frozen parameter has no state")
            if self.amsgrad and "max_exp_avg_sq" not in stt:
                raise ValueError(f"optimizer state #{i} ({k}) has no 'max_exp_avg_sq': it was saved without amsgrad, this trainer "
                                 "runs with amsgrad = True")
            for nm in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if self.amsgrad else ()):
                if tuple(stt[nm].shape) != tuple(self.params[k].shape):
                    raise ValueError(f"optimizer state #{i} ({nm}) has shape {tuple(stt[nm].shape)}, parameter {k} has "
                                     f"{tuple(self.params[k].shape)}: this checkpoint belongs to another model")
            new_m[k] = stt["exp_avg"].to(self.dev, torch.float32).contiguous().clone()
            new_v[k] = stt["exp_avg_sq"].to(self.dev, torch.float32).contiguous().clone()
            if self.amsgrad:
                new_x[k] = stt["max_exp_avg_sq"].to(self.dev, torch.float32).contiguous().clone()
            adam_step = int(stt["step"])
        self.m.update(new_m)
        self.v.update(new_v)
        self.vmax.update(new_x)
        if self._opt_state is not None:                         # the device counts the applied steps: it continues from the restored count
            s = self.scaler_state()
            self._write_opt_state(s["scale"], s["growth_tracker"], adam_step, s["skipped"])
        self.adam_step = adam_step
        g = osd["param_groups"][0]
        self.betas, self.eps = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])      # (shared by all groups)
        if self._groups is None:
            self.lr = float(g["lr"])
            return
        # per-group lr / weight_decay come back when the saved groups are this trainer's groups (same positions)
        pos = {k: i for i, k in enumerate(keys)}
        mine = [sorted(pos[k] for k in grp["names"]) for grp in self._groups]
        if mine == [sorted(int(i) for i in sg["params"]) for sg in osd["param_groups"]]:
            for grp, sg in zip(self._groups, osd["param_groups"]):
                grp["lr"], grp["weight_decay"] = float(sg["lr"]), float(sg.get("weight_decay", 0.0))
        else:
            import warnings
            warnings.warn(f"optimizer state with {len(osd['param_groups'])} parameter group(s) loaded into a trainer with "
                          f"{len(self._groups)} other group(s): moments, step count, betas and eps are restored, the groups' lr / "
                          "weight_decay stay this trainer's")


def step_seed_base(dropout_seed: int) -> int:
    """The base of the device-counted dropout seed: (base + tick) & (2^63 - 1) is `_step_seed()` at num_it = tick."""
    return (int(dropout_seed) * 1000003 + 1) & 0xFFFFFFFFFFFFFFFF


def capture_refusal(accum_steps: int, world_size: int, path: str = "trainer") -> Optional[str]:
    """Why a training step with these settings cannot be captured (None = it can). Needs no device."""
    if path != "trainer":
        return (f"capture: the {path} path runs the backward through torch.autograd, whose nodes allocate and read back; only "
                "FP32Trainer's own step is captured - this one stays eager")
    if accum_steps > 1:
        return (f"capture: accum_steps = {accum_steps}: an accumulation window spans several iterations with different launches "
                "(the first call's tensors become the sums, only the last one runs the optimiser); windows stay eager")
    if world_size > 1:
        return (f"capture: {world_size} ranks: the gradient exchange forks streams and runs gloo on the host, which a graph "
                "cannot hold; multi-rank steps stay eager")
    return None


BIAS_TABLE_MAX = 1 << 20        # entries of mode A's bias-correction table a capture accepts (vog_opt_bias_table)


class TrainSlot:
    """A captured training iteration of one trainer on one batch shape (`FP32Trainer.capture`).
    What changes from step to step lives in device memory: the batch (static tensors, one per key, refilled by `step`), the
    step block (vog_train_step: `tick` = the trainer's num_it, which numbers the dropout masks; `adam_step` = the applied
    plain-Adam updates, which picks the bias corrections from a host-built table; a sticky word for clamped sentence lengths),
    the learning-rate table (one float per parameter group; `step` rewrites it when a rate moved, with a stream-ordered copy
    outside the graph), and what was on the device already (the loss-scale block, the averaging block, p / m / v / vmax / avg).
    The graph is ONE chain on ONE stream: length guard, forward, loss, backward, optimiser, averaging, loss log + counts -
    kernel nodes only (recorded under the library's "kernel_fills" switch: with hipMemsetAsync / hipMemcpyAsync recorded as
    memset / memcpy nodes, back-to-back replays left stale data in zero-filled rows on this runtime); `step` launches it on the
    caller's current stream.
    `T` (default: the width of srl_arg_word_mask) bounds the language kernels; the guard clamps longer lengths to it in the
    static buffer and `check()` reports that. The losses of a replay go to row tick % log_rows of a device ring; `losses(n)`
    reads the last n replays' rows in one copy - so read at least every log_rows iterations.
    A slot is STALE - `step` raises VogError until the caller captures again - after set_param_groups, a changed frozen set,
    precision or operator switch, optimiser setting, another batch shape / key set / cached form, or replaced state tensors (a
    loaded checkpoint). An eager `trainer.step` in between is fine: the slot rewrites its counts from the trainer's.
    The library's per-thread launch counters (`*_launches`) count at capture, not per replay."""

    def __init__(self, tr: FP32Trainer, batch, T, log_rows: int, keep_graph: bool = False):
        if isinstance(log_rows, bool) or not isinstance(log_rows, int) or log_rows < 1:
            raise ValueError(f"log_rows = {log_rows!r}: an integer >= 1")
        lib, dev = tr.lib, tr.dev
        self.trainer, self.log_rows = tr, log_rows
        self.static = {k: (v.to(dev, torch.int64) if k in ("srl_arg_word_mask_len", "srl_arg_words_capture") else v.to(dev)).contiguous().clone()
                       for k, v in batch.items() if torch.is_tensor(v)}
        self._batch_sig = self.batch_signature(batch)
        lens = self.static.get("srl_arg_word_mask_len") if input_form(batch, WORD_KEYS) is None else None
        cap = self.static.get("srl_arg_words_capture") if lens is not None else None
        if lens is None:
            self.T = None
        else:
            width = int(self.static["srl_arg_word_mask"].shape[-1])
            self.T = width if T is None else int(T)
            if not 1 <= self.T <= width:
                raise ValueError(f"T = {T!r}: between 1 and the width of srl_arg_word_mask ({width})")
        self.loss_keys = list(tr.loss_fn.loss_keys)
        n_loss = len(self.loss_keys)
        self.block = torch.zeros(4, dtype=torch.int32, device=dev)       # vog_train_step: tick (2 words), adam_step, len_clamped
        self.ring = torch.zeros(log_rows, n_loss + 1, dtype=torch.float32, device=dev)
        self._dev_tick, self._dev_adam = -1, -1
        self._ticks = []                                                  # the ticks of the last replays (at most log_rows)
        self.replays = 0
        self.stream = torch.cuda.Stream(device=dev)
        cur = torch.cuda.current_stream(dev)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            # warm-up on the capture stream: fills the split-K buffer and the kernels' one-time function attributes. No
            # optimiser call on the trainer's state and num_it untouched: a captured trainer starts where an eager one does.
            for _ in range(2):
                with tr.precision():
                    _, grads = tr._gradients(self.static, False, T=self.T)
            self._grad_keys = frozenset(grads)
            del grads
            keys, spans = tr._opt_spans(self._grad_keys)
            self._prepare_state(keys)
            n_groups = 1 if spans is None else len(spans)
            self.lr_table = torch.zeros(max(n_groups, 1), dtype=torch.float32, device=dev)
            self._lrs = None
            self.bias_table, self.bias_len = None, 0
            if tr._opt_state is None:                                    # mode A: the bias corrections by update number
                n = ctypes.c_int(0)
                rc = lib.vog_opt_bias_table(tr.betas[0], tr.betas[1], None, 0, ctypes.byref(n))
                if rc == -1:
                    L.check(rc, "vog_opt_bias_table")
                if rc != -2 or n.value > BIAS_TABLE_MAX:
                    raise L.VogError(f"capture: betas {tr.betas} need a bias-correction table of more than 2^20 entries")
                host = (ctypes.c_float * (2 * n.value))()
                L.check(lib.vog_opt_bias_table(tr.betas[0], tr.betas[1], host, n.value, ctypes.byref(n)), "vog_opt_bias_table")
                self.bias_len = n.value
                self.bias_table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.float32).to(dev)
            self._warm_kernels()
        self.stream.synchronize()
        # pin the split-K buffer the warm-up left on this stream, if it left one: the graph points into it. (Without one no
        # product of this step takes the split-K path, and under capture the buffer cannot appear either.)
        held = ctypes.c_size_t(0)
        L.check(lib.vog_train_scratch_info(self.stream.cuda_stream, None, ctypes.byref(held), None), "vog_train_scratch_info")
        self._pinned = held.value > 0
        if self._pinned:
            L.check(lib.vog_train_pin_scratch(self.stream.cuda_stream, 1), "vog_train_pin_scratch")
        self._sync_counts()
        self._sync_lrs()
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
        self._keep_graph = bool(keep_graph)
        tr._dev = self
        try:
            L.check(lib.vog_train_set_ptr(b"drop_tick", L.ptr(self.block)), "vog_train_set_ptr")
            L.check(lib.vog_train_set_int(b"kernel_fills", 1), "vog_train_set_int")
            with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
                st = L.stream_ptr()
                L.check(lib.vog_train_tick(L.ptr(self.block), L.ptr(lens), 0 if lens is None else lens.numel(), self.T or 0, None,
                                           None, 0, 0, L.TICK_BEGIN, 0, L.ptr(cap), 0 if cap is None else cap.numel(), st),
                        "vog_train_tick")
                with tr.precision():
                    ld, grads = tr._gradients(self.static, False, T=self.T)
                if set(grads) != set(self._grad_keys):
                    raise L.VogError("capture: the step produced other gradients than its warm-up")
                tr._optimizer_step(grads)
                src = ld[self.loss_keys[0]]
                assert all(ld[k].data_ptr() == src.data_ptr() + 4 * i for i, k in enumerate(self.loss_keys))
                L.check(lib.vog_train_tick(L.ptr(self.block), None, 0, 0, src.data_ptr(), L.ptr(self.ring), log_rows, n_loss,
                                           L.TICK_END, 1 if tr._opt_state is None else 0, None, 0, st), "vog_train_tick")
                del ld, grads                                            # (alive until the last node that reads them is recorded)
        finally:
            lib.vog_train_set_ptr(b"drop_tick", None)
            lib.vog_train_set_int(b"kernel_fills", 0)
            tr._dev = None
        self._trainer_sig = self._signature()

    # ---- what the graph holds pointers to, made before the capture (an allocation inside it would live in the graph's pool
    # and be re-initialised by every replay)
    def _prepare_state(self, keys) -> None:
        tr = self.trainer
        total = 0
        for k in keys:
            p = tr.params[k]
            total += p.numel()
            if k not in tr.m:
                tr.m[k], tr.v[k] = torch.zeros_like(p), torch.zeros_like(p)
            if tr.amsgrad and k not in tr.vmax:
                tr.vmax[k] = torch.zeros_like(p)
            if tr.avg_mode is not None and k not in tr.avg:
                tr.avg[k] = torch.zeros_like(p)
        if tr.avg_mode is not None and tr._avg_state is None:
            tr._avg_state = torch.zeros(4, dtype=torch.int32, device=tr.dev)
        if tr._opt_state is not None:
            need = int(tr.lib.vog_opt_scratch_bytes(len(keys), total))
            if tr._opt_scratch is None or tr._opt_scratch.numel() < need:
                tr._opt_scratch = torch.empty(need, dtype=torch.uint8, device=tr.dev)

    def _warm_kernels(self) -> None:
        """One launch from each of the two source files the step's tail adds - the tick (train_step.hip) and the device-table
        optimiser (optim.hip, which also holds the averaging and every other instance of the apply kernel) - on throw-away
        tensors, so that the runtime loads those code objects before, not during, the capture."""
        tr, lib, st = self.trainer, self.trainer.lib, L.stream_ptr()
        blk = torch.zeros(4, dtype=torch.int32, device=tr.dev)
        t = [torch.zeros(4, dtype=torch.float32, device=tr.dev) for _ in range(5)]
        L.check(lib.vog_train_tick(L.ptr(blk), None, 0, 0, None, None, 0, 0, L.TICK_END, 0, None, 0, st), "vog_train_tick")
        arr = (L.OptTensor * 1)()
        arr[0].p, arr[0].g, arr[0].m, arr[0].v, arr[0].n = L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), 4
        ex = L.OptExArgs()
        a = ex.groups.base
        a.tensors, a.n_tensors, a.beta1, a.beta2, a.eps = arr, 1, tr.betas[0], tr.betas[1], tr.eps
        garr = (L.OptGroup * 1)()
        garr[0].first, garr[0].count = 0, 1
        ex.groups.groups, ex.groups.n_groups, ex.grad_scale = garr, 1, 1.0
        d = L.OptDevArgs()
        d.lr, d.step, d.bias, d.bias_len = L.ptr(t[4]), L.ptr(blk), L.ptr(t[4]), 1
        L.check(lib.vog_opt_step_dev_f32(ctypes.byref(ex), ctypes.byref(d), st), "vog_opt_step_dev_f32")
        self._keep_warm = (blk, t)

    def opt_dev_args(self, n_groups: int) -> "L.OptDevArgs":
        assert n_groups == self.lr_table.numel(), (n_groups, self.lr_table.numel())
        d = L.OptDevArgs()
        d.lr = L.ptr(self.lr_table)
        if self.trainer._opt_state is None:
            d.step, d.bias, d.bias_len = L.ptr(self.block), L.ptr(self.bias_table), self.bias_len
        return d

    @staticmethod
    def batch_signature(batch):
        form = input_form(batch, F32_KEYS[:2]), input_form(batch, WORD_KEYS)
        return (tuple(sorted((k, tuple(v.shape), str(v.dtype)) for k, v in batch.items() if torch.is_tensor(v))),
                tuple(None if f is None else f.name for f in form))

    def _signature(self):
        tr = self.trainer
        ptrs = [t.data_ptr() for d in (tr.params, tr.m, tr.v, tr.vmax, tr.avg) for t in d.values()]
        ptrs += [None if t is None else t.data_ptr() for t in (tr._opt_state, tr._avg_state, tr._opt_scratch)]
        wds = None if tr._groups is None else tuple((tuple(g["names"]), g["weight_decay"]) for g in tr._groups)
        return (tr._layout_epoch, tr.frozen, tr.amp, tr.bf16_gemm, tr.attn, tr.lstm, tr.lstm_amp, tr.gemm_amp, tr.qkv, tr.dropout,
                tr.dropout_seed, tr.optimizer, tr.amsgrad, tr.maximize, tr.accum_steps, tr.avg_mode, tr.avg_decay, tr.avg_warmup,
                tr.avg_start, tr.avg_every, tr.clip_norm, tr.loss_scale is None, tr.growth_interval, tr.growth_factor,
                tr.backoff_factor, tr.betas, tr.eps, wds, tuple(ptrs))

    def stale_reason(self, batch=None) -> Optional[str]:
        """Why this slot can no longer be replayed (None = it can)."""
        if self._signature() != self._trainer_sig:
            return ("the trainer changed after the capture (parameter groups, frozen set, precision / operator switches, optimiser "
                    "settings or state tensors)")
        if batch is not None and self.batch_signature(batch) != self._batch_sig:
            return "the batch has another shape, key set, dtype or cached form than the captured one"
        return None

    def matches(self, batch) -> bool:
        return self.batch_signature(batch) == self._batch_sig

    def _sync_counts(self) -> None:
        """The trainer's host counters -> the step block (after an eager step in between, a restored checkpoint, at capture);
        the sticky word is left alone."""
        tr = self.trainer
        if self._dev_tick == tr.num_it and (tr._opt_state is not None or self._dev_adam == tr.adam_step):
            return
        h = L.TrainStep(tick=tr.num_it, adam_step=tr.adam_step, len_clamped=0)
        self.block[:3].copy_(torch.frombuffer(bytearray(bytes(h)), dtype=torch.int32)[:3])
        self._dev_tick, self._dev_adam = tr.num_it, tr.adam_step

    def _sync_lrs(self) -> None:
        tr = self.trainer
        spans = tr._opt_spans(self._grad_keys)[1]
        lrs = [tr.lr] if spans is None else [sp[2] for sp in spans]
        if lrs != self._lrs:
            self.lr_table.copy_(torch.tensor(lrs, dtype=torch.float32))
            self._lrs = lrs

    def step(self, batch, longest=None) -> None:
        """One iteration on `batch` (same keys and shapes as the captured one): per-key copies into the static tensors, then
        ONE graph launch. Returns nothing - nothing is read back (`losses`, `check`). longest: the longest sentence if the
        caller knows it on the host; beyond T it is a ValueError before any launch."""
        tr = self.trainer
        if longest is not None and self.T is not None and int(longest) > self.T:
            raise ValueError(f"longest = {int(longest)} exceeds the T = {self.T} this slot was captured for")
        why = self.stale_reason(batch)
        if why:
            raise L.VogError(f"TrainSlot.step: stale slot - {why}; capture again")
        for k, dst in self.static.items():
            dst.copy_(batch[k], non_blocking=True)
        self._sync_counts()
        self._sync_lrs()
        self.graph.replay()
        self._ticks.append(tr.num_it)
        del self._ticks[:-self.log_rows]
        tr.num_it += 1
        self._dev_tick += 1
        if tr._opt_state is None:
            tr.adam_step += 1
            self._dev_adam += 1
        self.replays += 1

    def losses(self, n: Optional[int] = None):
        """The loss dicts ({key: 0-dim fp32 tensor on the host}) of the last n replays (None: all the ring still holds), oldest
        first: ONE copy of the ring. A row whose marker is not its replay's was overwritten (more than log_rows iterations
        since): VogError."""
        ticks = self._ticks if n is None else self._ticks[len(self._ticks) - int(n):] if n else []
        if n is not None and int(n) > len(self._ticks):
            raise L.VogError(f"losses({n}): the ring holds the last {len(self._ticks)} replays")
        if not ticks:
            return []
        ring = self.ring.cpu()
        marks = ring.view(torch.int32)[:, len(self.loss_keys)].tolist()
        out = []
        for t in ticks:
            r = t % self.log_rows
            if (marks[r] & 0xFFFFFFFF) != ((t + 1) & 0xFFFFFFFF):
                raise L.VogError(f"losses: the row of iteration {t} was overwritten (read at least every {self.log_rows} iterations)")
            out.append({k: ring[r, i] for i, k in enumerate(self.loss_keys)})
        return out

    def check(self) -> None:
        """Reads the sticky word (one 16-byte copy): VogError if a replay had to clamp a sentence length to T - that step
        trained on a truncated sentence."""
        if int(self.block.cpu()[3]) != 0:
            raise L.VogError(f"TrainSlot.check: a batch carried a sentence longer than T = {self.T}; its length was clamped and "
                             "that step computed a truncated sentence. Capture with a larger T")

    def nodes(self) -> Optional[int]:
        """The number of nodes of the captured graph (captured with keep_graph=True; None otherwise)."""
        if not self._keep_graph:
            return None
        n = ctypes.c_int(0)
        L.check(self.trainer.lib.vog_graph_node_count(self.graph.raw_cuda_graph(), ctypes.byref(n)), "vog_graph_node_count")
        return n.value

    def release(self) -> None:
        """Unpins the capture stream's split-K buffer and marks the slot stale for good (the graph must not be replayed
        afterwards). Also runs when the slot is dropped: torch hands stream handles out again, and a later user of this one
        must not inherit the pin."""
        if getattr(self, "_pinned", False):
            self.trainer.lib.vog_train_pin_scratch(self.stream.cuda_stream, 0)
            self._pinned = False
        self._trainer_sig = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class SmoothenDict:
    """Exponentially smoothed loss values with bias correction (utils/trn_utils.py:228-262: SmoothenValue / SmoothenDict)."""

    def __init__(self, keys, beta: float):
        self.keys, self.beta, self.n = list(keys), beta, 0
        self.mov = {k: 0.0 for k in self.keys}
        self.smooth = {k: 0.0 for k in self.keys}

    def add_value(self, d):
        self.n += 1
        for k in self.keys:
            self.mov[k] = self.beta * self.mov[k] + (1 - self.beta) * float(d[k])
            self.smooth[k] = self.mov[k] / (1 - self.beta ** self.n)
