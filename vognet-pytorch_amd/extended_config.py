"""Config surface of the VOGNet forward path.

Mirrors the *interface* of the reference config layer (reference
code/extended_config.py:36-81 `update_from_dict`, configs/anet_srl_cfg.yml for
key names and defaults) without depending on yacs (not installed here): a small
attribute-dict `CfgNode` with freeze/defrost, dotted-key overrides that assert
the key exists and that the new value has the type of the default.

Only the keys the forward path, the prediction head and the CLI read are kept
under the same names; dataset file paths are retained as inert strings so that
`--ds.some_path=...` overrides of a reference command line still parse.
"""
from __future__ import annotations

import ast
import copy
from typing import Any, Dict


class CfgNode(dict):
    """Attribute-access dict with yacs-like freeze semantics."""

    _FROZEN = "__frozen__"

    def __init__(self, init: Dict[str, Any] | None = None):
        super().__init__()
        object.__setattr__(self, CfgNode._FROZEN, False)
        for k, v in (init or {}).items():
            dict.__setitem__(self, k, CfgNode(v) if isinstance(v, dict) else v)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def __setitem__(self, key, value):
        if object.__getattribute__(self, CfgNode._FROZEN):
            raise AttributeError(f"cfg is frozen; cannot set {key!r}")
        if isinstance(value, dict) and not isinstance(value, CfgNode):
            value = CfgNode(value)
        dict.__setitem__(self, key, value)

    def _set_frozen(self, flag: bool):
        object.__setattr__(self, CfgNode._FROZEN, flag)
        for v in self.values():
            if isinstance(v, CfgNode):
                v._set_frozen(flag)

    def freeze(self):
        self._set_frozen(True)

    def defrost(self):
        self._set_frozen(False)

    def is_frozen(self) -> bool:
        return object.__getattribute__(self, CfgNode._FROZEN)

    def clone(self) -> "CfgNode":
        return CfgNode(self.to_dict())

    def to_dict(self) -> Dict[str, Any]:
        return {k: (v.to_dict() if isinstance(v, CfgNode) else copy.deepcopy(v))
                for k, v in self.items()}

    def __deepcopy__(self, memo):
        return self.clone()


# Defaults: same keys / values as the reference yaml (configs/anet_srl_cfg.yml:1-131).
_DEFAULTS: Dict[str, Any] = {
    "ds_name": "anet",
    "ds": {
        "seg_feature_root": "data/anet/rgb_motion_1d",
        "exp_setting": "gt5",
        "gt5": {
            "proposal_h5": "data/anet/anet_detection_vg_fc6_feat_gt5_rois.h5",
            "feature_root": "data/anet/fc6_feat_5rois",
            "num_prop_per_frm": 5,
        },
        "p100": {
            "proposal_h5": "data/anet/anet_detection_vg_fc6_feat_100rois_resized.h5",
            "feature_root": "data/anet/fc6_feat_100rois",
            "num_prop_per_frm": 100,
        },
        "resized_width": 720,
        "resized_height": 405,
        "num_sampled_frm": 10,
        "max_gt_box": 100,
        "t_attn_size": 480,
        "max_seq_length": 20,
        "anet_cap_file": "data/anet_cap_ent_files/anet_captions_all_splits.json",
        "anet_ent_annot_file": "data/anet_cap_ent_files/anet_ent_cls_bbox_trainval.json",
        "anet_ent_split_file": "data/anet_cap_ent_files/dic_anet.json",
        "include_srl_args": ["ARG0", "ARG1", "ARG2", "ARGM-LOC"],
        "arg_vocab_file": "data/anet_srl_files/arg_vocab.pkl",
        "trn_ann_file": "data/anet_cap_ent_files/csv_dir/train_postproc.csv",
        "val_ann_file": "data/anet_cap_ent_files/csv_dir/val_postproc.csv",
        "trn_ds4_dicts": "data/anet_srl_files/trn_srl_obj_to_index_dict.json",
        "val_ds4_dicts": "data/anet_srl_files/val_srl_obj_to_index_dict.json",
        "trn_ds4_inds": "data/anet_srl_files/trn_asrl_annots.csv",
        "val_ds4_inds": "data/anet_srl_files/val_asrl_annots.csv",
        "trn_sample": "ds4_random",
        "val_sample": "ds4",
        "trn_num_vid_sample": 4,
        "val_num_vid_sample": 4,
        "conc_type": "spat",
        "cs_shuffle": True,
        "none_word": "<none>",
    },
    "mdl": {
        "name": "vog",
        "seg_feat_dim": 3072,
        "prop_feat_dim": 2048,
        "input_encoding_size": 512,
        "use_vis_msk": True,
        "rnn": {"rnn_size": 1024, "num_layers": 2, "drop_prob_lm": 0.5},
        "vsrl": {"prop_encode_size": 256, "seg_encode_size": 256,
                 "lang_encode_size": 256},
        "obj_tx": {"use_ddp": False, "to_use": True, "n_layers": 1,
                   "n_heads": 3, "attn_drop": 0.2, "use_rel": False,
                   "one_frm": False},
        "mul_tx": {"use_ddp": False, "to_use": True, "n_layers": 1,
                   "n_heads": 3, "attn_drop": 0.2, "use_rel": False,
                   "one_frm": True, "cross_frm": False},
    },
    "loss": {"only_vid_loss": False, "loss_lambda": 1, "loss_margin": 0.1,
             "loss_margin_vid": 0.5, "loss_type": "bce"},
    "misc": {"tmp_path": "tmp", "prop_thresh": 0.0, "exclude_bgd_det": False,
             "add_prop_to_region": False, "ctx_for_seg_feats": 0,
             "srl_arg_length": 5, "box_per_srl_arg": 4},
    "train": {"lr": 1e-4, "epochs": 10, "bs": 4, "nw": 4, "bsv": 4, "nwv": 4,
              "resume": True, "resume_path": "", "load_opt": False,
              "load_normally": True, "strict_load": True,
              "use_reduce_lr_plateau": False, "verbose": False,
              "prob_thresh": 0.2},
    "log": {"deb_it": 2},
    "local_rank": 0,
    "do_dist": False,
    "do_dp": False,
    "num_gpus": 1,
    "only_val": False,
    "only_test": False,
    "run_final_val": True,
    "overfit_batch": False,
    # build-specific (not in the reference yaml): arithmetic type of the two
    # transformers' MFMA contractions ("auto" | "bf16" | "f16"); fp32 accumulate always. "auto" = bf16 for
    # single-layer stacks (the reference default, BASELINE.json config 2), f16 when a stack has more layers
    # (engine.model_desc_from_cfg: the 1e-3 bound against the full-size 3-layer golden).
    # batch_requests: Evaluator.forward serves this many loader batches as ONE forward (dynamic batching; 1 = off)
    # train_amp: precision of the Learner's training step - "" = fp32, "bf16" | "f16" = mixed precision (FP32Trainer(amp=...));
    # "f16" is accepted only with a loss scale
    # train_loss_scale: "" = none, "dynamic" = torch.amp.GradScaler's schedule from 2^16 (a step with a non-finite gradient is
    # skipped and the scale halved, 2000 clean steps double it), a number as text ("1024") = the same schedule from that scale
    # train_clip_norm: the gradients' global L2 norm is clipped to this (torch.nn.utils.clip_grad_norm_); 0.0 = off. With either
    # key set the optimiser step measures the gradients on the device and skips a non-finite step (vog_opt_step_f32)
    # train_freeze: a comma list of stages the Learner's training step does not train ("lang", "enc", "obj": engine.TRAIN_STAGES;
    # "" = everything is trained). A frozen stage gets no gradient and no Adam state (FP32Trainer(freeze=...)); the trainer takes a
    # cached input form for a stage that is frozen whole, but main_dist's training loaders keep feeding the raw keys
    # train_optimizer: "adam" (a parameter group's weight_decay is the L2 form) | "adamw" (decoupled decay); train_amsgrad: the
    # AMSGrad denominator; train_accum_steps: micro-batches per optimiser step (gradient accumulation; an epoch's last, shorter
    # window is applied with its own count) - FP32Trainer(optimizer=, amsgrad=, accum_steps=)
    # train_plateau_factor / train_plateau_patience (read with cfg.train.use_reduce_lr_plateau): ReduceLROnPlateau's factor and
    # patience on the first validation metric, stepped once per epoch (the reference reads cfg.reduce_factor / cfg.patience,
    # which none of its configs defines: these two keys stand in for them)
    # device_metrics: Evaluator.forward scores the prediction records on the device (vog_ground_metrics) instead of re-reading
    # its own pickle on the host; val_pickle: False (with device_metrics) = no prediction pickle and no record exchange
    # val_graph: Evaluator.forward serves every full-shape batch with a fed graph slot whose graph ends in the loss, the metrics
    # and the validation log (one transfer + one launch per step; engine.FedPipeline(..., epilogue=)); not with batch_requests > 1
    # query_bank (read only with val_graph): the per-query rows of the loader's batches live in a device-resident
    # dat_loader_simple.QueryBank; a step writes the rows' numbers and the step number, the graph gathers the rows
    # lang_bank (needs query_bank and val_graph, refused otherwise: `check_hip_options`): the query bank's word-level columns are
    # replaced by the language chain's results under the current weights (dat_loader_simple.LangBank, encoded once per checkpoint
    # at the pass's (B, T_max)); the slots' forwards start behind the BiLSTM. Off by default: its gain is workload-dependent
    # weight_refresh: how changed parameters reach a finalized inference engine - "host" = VogEngine.load_state_dict (through
    # the CPU, every buffer reallocated, captured slots refuse afterwards), "device" = VogEngine.refresh_from_device (the weight
    # images are rewritten in place by HIP pack kernels from the fp32 device parameters; captured slots and the evaluator's
    # validation-graph pipeline stay valid). Read by AnetBaseMdl.engine() and Learner._sync_model
    # train_avg: "" = off | "ema" | "swa": the training step keeps an average of the parameters on the device, updated behind every
    # applied optimiser step (vog_opt_average_f32; a step skipped on overflow does not average) - FP32Trainer(avg=, avg_decay=,
    # avg_warmup=, avg_start=, avg_every=). train_avg_decay: EMA's decay; train_avg_warmup: cap it at (1 + n) / (10 + n);
    # train_avg_start / train_avg_every: average on applied step s when s >= start and (s - start) % every == 0.
    # train_avg_eval (needs train_avg): Learner.validate - and with it best_met and the plateau schedule's metric - runs on the
    # AVERAGED weights; `main_dist --only_val` then evaluates the averaged weights of the checkpoint
    # train_attn: the attention operator of the training step's encoder layers (Learner and the autograd path) - "materialized" =
    # vog_attn_f32 (the [S, N, N] probabilities of one head at a time in scratch) | "fused" = vog_attn_fused_f32 (online softmax,
    # O(N) scratch, one forward and two backward launches for all heads) | "fused_pipe" = the same operator on its pipelined
    # kernels (two LDS buffers, one barrier per staged tile; the bits and the scratch of "fused") - FP32Trainer(attn=)
    # train_lstm: the fp32 BiLSTM recurrence of the training step (Learner and the autograd path) - "stepwise" = a recurrent
    # product and a cell launch per layer, direction and step | "fused" = one launch per layer and step for both directions
    # (no effect under train_amp, whose recurrence is fused already) - FP32Trainer(lstm=)
    # train_lstm_amp: the BiLSTM recurrence under train_amp - "tile" = a workgroup owns 16 units, a wave a gate and all of K |
    # "split" = K split over the waves of a workgroup (same operands, another order of the fp32 sums; no effect without
    # train_amp) - FP32Trainer(lstm_amp=)
    # train_gemm_amp: the vector tile products under train_amp - "tile" = the single-buffer 128 x 64 kernel | "pipe" = the pipelined
    # kernel (two LDS buffers, 64-wide K episodes, one barrier each; the same bits; no effect without train_amp) -
    # FP32Trainer(gemm_amp=)
    # lstm_wide: the persistent BiLSTM layer kernel also serves language chains of 17 .. 32 sentences (sep at bs 5 .. 8, svsq /
    # spat / temp at bs 17 .. 32, eight batched bs-4 requests) instead of the step launches (context option "lstm_wide";
    # VogEngine applies it; off by default)
    # train_qkv: the Q / K / V projections of mul_tx's layer 0 in the training step (Learner and the autograd path) - "dense" = the
    # products over every [vis | lang] token | "factored" = the products over the distinct obj_tx rows and over the argument
    # vectors, added per token (another order of the fp32 sums; no effect on a model without mul_tx) - FP32Trainer(qkv=)
    # train_graph: Learner.train_epoch captures the training iteration on the first batch of the epoch's shape and replays it with
    # one graph launch per batch (FP32Trainer.capture); other shapes run the eager step. Off by default
    "hip": {"tx_dtype": "auto", "use_graph": True, "batch_requests": 1, "train_amp": "", "device_metrics": False,
            "val_pickle": True, "train_loss_scale": "", "train_clip_norm": 0.0, "val_graph": False, "query_bank": False,
            "lang_bank": False, "train_freeze": "", "train_optimizer": "adam", "train_amsgrad": False, "train_accum_steps": 1,
            "train_plateau_factor": 0.1, "train_plateau_patience": 10, "weight_refresh": "host", "train_avg": "",
            "train_avg_decay": 0.999, "train_avg_warmup": False, "train_avg_start": 1, "train_avg_every": 1, "train_avg_eval": False,
            "train_attn": "materialized", "train_lstm": "stepwise", "train_lstm_amp": "tile",
            "train_gemm_amp": "tile", "lstm_wide": False, "train_qkv": "dense", "train_graph": False},
}

key_maps: Dict[str, str] = {}

# text keys whose value may read as a number ("dynamic" | "1024"): update_from_dict keeps the text
_NUMBER_AS_TEXT = frozenset({"hip.train_loss_scale"})


def get_default_cfg() -> CfgNode:
    """Fresh, unfrozen copy of the default config (reference: module-level
    `cfg` built at import time, code/extended_config.py:7-11)."""
    c = CfgNode(copy.deepcopy(_DEFAULTS))
    c.comm = CfgNode()
    return c


def _decode_cfg_value(v: Any) -> Any:
    """CLI strings -> python literals (yacs `_decode_cfg_value` behaviour)."""
    if not isinstance(v, str):
        return v
    try:
        return ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return v


def update_from_dict(cfg: CfgNode, dct: Dict[str, Any],
                     key_maps: Dict[str, str] | None = None) -> CfgNode:
    """Dotted-key override with the reference's checks
    (code/extended_config.py:36-81): unknown key -> AssertionError, type
    mismatch with the default -> AssertionError. One exception, for the keys
    of _NUMBER_AS_TEXT: their text may be a number, which is kept as text."""
    key_maps = key_maps or {}
    dct = dict(dct)
    for full_key in list(dct.keys()):
        if full_key in key_maps:
            dct[key_maps[full_key]] = dct.pop(full_key)
    for full_key, v in dct.items():
        key_list = full_key.split(".")
        d = cfg
        for subkey in key_list[:-1]:
            assert subkey in d, f"key {full_key} doesnot exist"
            d = d[subkey]
        subkey = key_list[-1]
        assert subkey in d, f"key {full_key} doesnot exist"
        value = _decode_cfg_value(v)
        old = d[subkey]
        if isinstance(old, float) and isinstance(value, int) and not isinstance(value, bool):
            value = float(value)
        if full_key in _NUMBER_AS_TEXT and isinstance(v, str) and isinstance(value, (int, float)) and not isinstance(value, bool):
            value = v                                  # --hip.train_loss_scale=1024 stays the text "1024"
        assert isinstance(value, type(old)), (
            f"type mismatch for {full_key}: {type(value)} vs {type(old)}")
        d[subkey] = value
    return cfg


TRAIN_FREEZE_STAGES = ("lang", "enc", "obj")            # (engine.TRAIN_STAGES' names; this module imports no device code)


def parse_train_freeze(text) -> tuple:
    """cfg.hip.train_freeze ("" | a comma list of stage names) -> the stage names; an unknown name is a ValueError."""
    if text in ("", None):
        return ()
    if not isinstance(text, str):
        raise ValueError(f"cfg.hip.train_freeze = {text!r}: a comma list of {', '.join(TRAIN_FREEZE_STAGES)}")
    names = tuple(x.strip() for x in text.split(",") if x.strip())
    for n in names:
        if n not in TRAIN_FREEZE_STAGES:
            raise ValueError(f"cfg.hip.train_freeze = {text!r}: unknown stage '{n}' (one of {', '.join(TRAIN_FREEZE_STAGES)})")
    return tuple(dict.fromkeys(names))


WEIGHT_REFRESH_MODES = ("host", "device")


def parse_weight_refresh(hip) -> str:
    """cfg.hip.weight_refresh -> "host" | "device"; anything else is a ValueError. Absent (a reference config): "host"."""
    mode = hip.get("weight_refresh", "host") if hasattr(hip, "get") else "host"
    if mode not in WEIGHT_REFRESH_MODES:
        raise ValueError(f"cfg.hip.weight_refresh = {mode!r}: one of {', '.join(WEIGHT_REFRESH_MODES)}")
    return mode


TRAIN_OPTIMIZERS = ("adam", "adamw")                     # (train.OPTIMIZERS; this module imports no device code)


def parse_train_optimizer(hip) -> dict:
    """The optimiser keys of cfg.hip -> {optimizer, amsgrad, accum_steps, plateau_factor, plateau_patience}; a value that cannot
    run is a ValueError that names its key. Absent keys (a reference config without them) take the defaults."""
    get = hip.get if hasattr(hip, "get") else (lambda k, d: d)
    opt, ams, acc = get("train_optimizer", "adam"), get("train_amsgrad", False), get("train_accum_steps", 1)
    factor, patience = get("train_plateau_factor", 0.1), get("train_plateau_patience", 10)
    if opt not in TRAIN_OPTIMIZERS:
        raise ValueError(f"cfg.hip.train_optimizer = {opt!r}: one of {', '.join(TRAIN_OPTIMIZERS)}")
    if not isinstance(ams, bool):
        raise ValueError(f"cfg.hip.train_amsgrad = {ams!r}: True or False")
    if isinstance(acc, bool) or not isinstance(acc, int) or acc < 1:
        raise ValueError(f"cfg.hip.train_accum_steps = {acc!r}: an integer >= 1")
    if isinstance(factor, bool) or not isinstance(factor, (int, float)) or not 0.0 < factor < 1.0:
        raise ValueError(f"cfg.hip.train_plateau_factor = {factor!r}: a number in (0, 1)")
    if isinstance(patience, bool) or not isinstance(patience, int) or patience < 0:
        raise ValueError(f"cfg.hip.train_plateau_patience = {patience!r}: an integer >= 0")
    return {"optimizer": opt, "amsgrad": ams, "accum_steps": acc, "plateau_factor": float(factor), "plateau_patience": patience}


TRAIN_AVG_MODES = ("ema", "swa")                         # (train.AVG_MODES; this module imports no device code)


def parse_train_avg(hip) -> dict:
    """The weight-averaging keys of cfg.hip -> {avg (None = off), decay, warmup, start, every, eval}; a value that cannot run is a
    ValueError that names its key, and so is train_avg_eval without train_avg. Absent keys take the defaults (everything off)."""
    get = hip.get if hasattr(hip, "get") else (lambda k, d: d)
    mode, decay, warm = get("train_avg", ""), get("train_avg_decay", 0.999), get("train_avg_warmup", False)
    start, every, ev = get("train_avg_start", 1), get("train_avg_every", 1), get("train_avg_eval", False)
    if mode not in ("", None) + TRAIN_AVG_MODES:
        raise ValueError(f"cfg.hip.train_avg = {mode!r}: '' (off) or one of {', '.join(TRAIN_AVG_MODES)}")
    if isinstance(decay, (bool, str)) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:
        raise ValueError(f"cfg.hip.train_avg_decay = {decay!r}: a number in [0, 1]")
    if not isinstance(warm, bool):
        raise ValueError(f"cfg.hip.train_avg_warmup = {warm!r}: True or False")
    for key, val in (("train_avg_start", start), ("train_avg_every", every)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 1:
            raise ValueError(f"cfg.hip.{key} = {val!r}: an integer >= 1 (applied optimiser steps)")
    if not isinstance(ev, bool):
        raise ValueError(f"cfg.hip.train_avg_eval = {ev!r}: True or False")
    if ev and not mode:
        raise ValueError("cfg.hip.train_avg_eval = True needs cfg.hip.train_avg = 'ema' | 'swa': without it there are no averaged "
                         "weights to evaluate")
    return {"avg": mode or None, "decay": float(decay), "warmup": warm, "start": start, "every": every, "eval": ev}


def parse_train_attn(hip) -> str:
    """cfg.hip.train_attn -> 'materialized' | 'fused' | 'fused_pipe' (a config without the key: 'materialized')."""
    v = hip.get("train_attn", "materialized") if hasattr(hip, "get") else "materialized"
    if not isinstance(v, str) or v not in ("materialized", "fused", "fused_pipe"):
        raise ValueError(f"cfg.hip.train_attn = {v!r}: one of 'materialized', 'fused', 'fused_pipe'")
    return v


def parse_train_lstm(hip) -> str:
    """cfg.hip.train_lstm -> 'stepwise' | 'fused' (a config without the key: 'stepwise')."""
    v = hip.get("train_lstm", "stepwise") if hasattr(hip, "get") else "stepwise"
    if v not in ("stepwise", "fused"):
        raise ValueError(f"cfg.hip.train_lstm = {v!r}: one of 'stepwise', 'fused'")
    return v


def parse_train_lstm_amp(hip) -> str:
    """cfg.hip.train_lstm_amp -> 'tile' | 'split' (a config without the key: 'tile')."""
    v = hip.get("train_lstm_amp", "tile") if hasattr(hip, "get") else "tile"
    if not isinstance(v, str) or v not in ("tile", "split"):
        raise ValueError(f"cfg.hip.train_lstm_amp = {v!r}: one of 'tile', 'split'")
    return v


def parse_train_gemm_amp(hip) -> str:
    """cfg.hip.train_gemm_amp -> 'tile' | 'pipe' (a config without the key: 'tile')."""
    v = hip.get("train_gemm_amp", "tile") if hasattr(hip, "get") else "tile"
    if not isinstance(v, str) or v not in ("tile", "pipe"):
        raise ValueError(f"cfg.hip.train_gemm_amp = {v!r}: one of 'tile', 'pipe'")
    return v


def parse_train_qkv(hip) -> str:
    """cfg.hip.train_qkv -> 'dense' | 'factored' (a config without the key: 'dense')."""
    v = hip.get("train_qkv", "dense") if hasattr(hip, "get") else "dense"
    if not isinstance(v, str) or v not in ("dense", "factored"):
        raise ValueError(f"cfg.hip.train_qkv = {v!r}: one of 'dense', 'factored'")
    return v


def parse_train_graph(hip) -> bool:
    """cfg.hip.train_graph -> True | False (a config without the key: False)."""
    v = hip.get("train_graph", False) if hasattr(hip, "get") else False
    if not isinstance(v, bool):
        raise ValueError(f"cfg.hip.train_graph = {v!r}: True or False")
    return v


def check_hip_options(cfg) -> None:
    """Combinations of the cfg.hip switches that cannot run. hip.lang_bank: the language bank is the query bank's tables with the
    word-level columns replaced, gathered by the validation graph - without hip.query_bank and hip.val_graph nothing would build
    or read it, and silently ignoring the switch would report timings of another path. hip.train_freeze: stage names only.
    The optimiser keys: `parse_train_optimizer`. hip.weight_refresh: `parse_weight_refresh`. The averaging keys: `parse_train_avg`.
    hip.train_attn: `parse_train_attn`. hip.train_lstm: `parse_train_lstm`. hip.train_lstm_amp: `parse_train_lstm_amp`.
    hip.train_gemm_amp: `parse_train_gemm_amp`. hip.train_qkv: `parse_train_qkv`. hip.train_graph: `parse_train_graph`."""
    hip = cfg.get("hip", None) if hasattr(cfg, "get") else None
    if hip is None:
        return
    parse_train_freeze(hip.get("train_freeze", ""))
    parse_train_optimizer(hip)
    parse_weight_refresh(hip)
    parse_train_avg(hip)
    parse_train_attn(hip)
    parse_train_lstm(hip)
    parse_train_lstm_amp(hip)
    parse_train_gemm_amp(hip)
    parse_train_qkv(hip)
    parse_train_graph(hip)
    if bool(hip.get("lang_bank", False)) and not (bool(hip.get("query_bank", False)) and bool(hip.get("val_graph", False))):
        raise ValueError("cfg.hip.lang_bank needs cfg.hip.query_bank = True and cfg.hip.val_graph = True (the language bank replaces "
                         "the query bank's word-level columns and is gathered by the validation graph)")


def post_proc_config(cfg: CfgNode) -> CfgNode:
    check_hip_options(cfg)
    return cfg


def num_prop_per_frm(cfg: CfgNode) -> int:
    """comm.num_prop_per_frm as the data layer derives it
    (reference code/dat_loader_simple.py: cfg.ds[exp_setting].num_prop_per_frm)."""
    return int(cfg.ds[cfg.ds.exp_setting].num_prop_per_frm)
