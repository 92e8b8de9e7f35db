"""`Learner` with the reference's surface (utils/trn_utils.py:265-860) over the device training step:

    learn = Learner(uid, data, mdl, loss_fn, cfg, eval_fn, opt_fn=None, device=...)
    learn.fit(epochs, lr) | learn.validate(db) | learn.testing(db) | learn.save_model_dict() | learn.load_model_dict(...)

`data` carries `.path`, `.train_dl`, `.valid_dl`, `.test_dl` (the reference's DataWrap, utils/trn_utils.py:250-262). Files land where
the reference puts them (init_log_dirs :341-368): `<path>/txt_logs/<uid>.txt`, `<path>/models/<uid>.pth`,
`<path>/predictions/<uid>/<dl_name>_0.pkl`. The iteration itself is `train.FP32Trainer.step` (forward -> loss -> backward ->
gradient all-reduce -> Adam on the device); validation is the evaluator on the inference model (16-bit HIP forward) carrying the
trainer's current weights. `opt_fn` is accepted for signature compatibility: the optimizer is the reference's Adam(betas (0.9, 0.99))
(code/main_dist.py:55) as `vog_opt_step_f32`, with loss scaling and gradient clipping from `cfg.hip.train_loss_scale` /
`train_clip_norm`; `fit(epochs, lr, params_opt_dict)` maps the reference's parameter groups onto it (vog_opt_step_groups_f32) and
`cfg.hip.train_freeze` freezes whole stages; `cfg.hip.train_optimizer` / `train_amsgrad` / `train_accum_steps` select AdamW, AMSGrad
and gradient accumulation (vog_opt_step_ex_f32, vog_opt_accum_f32), and `prepare_scheduler` / `scheduler_step` step torch's own
LambdaLR / ReduceLROnPlateau (`cfg.train.use_reduce_lr_plateau`) once per epoch over the trainer's learning rates.
`cfg.hip.train_avg` = ema | swa keeps an average of the parameters on the device (vog_opt_average_f32) and saves it as
`averaging_state_dict` beside the trained `model_state_dict`; with `cfg.hip.train_avg_eval` validation runs on the averaged weights. Progress bars, tensorboard and the python logger are not reproduced.
"""
from __future__ import annotations

import json
import time
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import dist as D
from .train import FP32Trainer, SmoothenDict, parse_clip_norm, parse_loss_scale


def _hip(cfg, key, default):
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return hip.get(key, default) if hasattr(hip, "get") else default


def train_loss_scale(cfg):
    """cfg.hip.train_loss_scale ('' | 'dynamic' | a positive number as text) -> None | 'dynamic' | float: FP32Trainer's loss_scale."""
    v = _hip(cfg, "train_loss_scale", "")
    if v in ("", None):
        return None
    if isinstance(v, str) and v.strip().lower() == "dynamic":
        return "dynamic"
    try:
        return parse_loss_scale(float(v) if isinstance(v, str) else v)
    except ValueError:
        raise ValueError(f"cfg.hip.train_loss_scale = {v!r}: '', 'dynamic' or a positive number") from None


def train_clip_norm(cfg) -> Optional[float]:
    """cfg.hip.train_clip_norm (0 = off) -> None | the largest gradient norm: FP32Trainer's clip_norm."""
    v = _hip(cfg, "train_clip_norm", 0.0)
    if isinstance(v, (bool, str)) or not isinstance(v, (int, float)) or not 0.0 <= v < float("inf"):
        raise ValueError(f"cfg.hip.train_clip_norm = {v!r}: 0 (off) or a positive number")
    return parse_clip_norm(float(v)) if v > 0.0 else None


def train_amp(cfg) -> Optional[str]:
    """cfg.hip.train_amp -> the trainer's precision mode (None = fp32). A reference yacs config without a `hip` section is fp32.
    'f16' needs a loss scale (cfg.hip.train_loss_scale): unscaled, its gradients underflow."""
    mode = _hip(cfg, "train_amp", "")
    if mode in ("", None):
        return None
    if mode == "f16":
        if train_loss_scale(cfg) is None:
            raise ValueError("cfg.hip.train_amp = 'f16' needs loss scaling: set cfg.hip.train_loss_scale ('dynamic' or a number), train "
                             "f16 through autograd under torch.autocast('cuda', dtype=torch.float16) with "
                             "torch.amp.GradScaler('cuda'), or use 'bf16'")
        return mode
    if mode != "bf16":
        raise ValueError(f"cfg.hip.train_amp = {mode!r}: one of '', 'bf16', 'f16'")
    return mode


def train_freeze(cfg) -> tuple:
    """cfg.hip.train_freeze -> the frozen stage names: FP32Trainer's freeze."""
    from .extended_config import parse_train_freeze
    return parse_train_freeze(_hip(cfg, "train_freeze", ""))


def train_optimizer(cfg) -> dict:
    """The optimiser keys of cfg.hip, checked (extended_config.parse_train_optimizer)."""
    from .extended_config import parse_train_optimizer
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_optimizer(hip)


def train_avg(cfg) -> dict:
    """The weight-averaging keys of cfg.hip, checked (extended_config.parse_train_avg)."""
    from .extended_config import parse_train_avg
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_avg(hip)


def train_attn(cfg) -> str:
    """cfg.hip.train_attn, checked (extended_config.parse_train_attn): FP32Trainer's attn."""
    from .extended_config import parse_train_attn
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_attn(hip)


def train_lstm(cfg) -> str:
    """cfg.hip.train_lstm, checked (extended_config.parse_train_lstm): FP32Trainer's lstm."""
    from .extended_config import parse_train_lstm
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_lstm(hip)


def train_lstm_amp(cfg) -> str:
    """cfg.hip.train_lstm_amp, checked (extended_config.parse_train_lstm_amp): FP32Trainer's lstm_amp."""
    from .extended_config import parse_train_lstm_amp
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_lstm_amp(hip)


def train_gemm_amp(cfg) -> str:
    """cfg.hip.train_gemm_amp, checked (extended_config.parse_train_gemm_amp): FP32Trainer's gemm_amp."""
    from .extended_config import parse_train_gemm_amp
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_gemm_amp(hip)


def train_qkv(cfg) -> str:
    """cfg.hip.train_qkv, checked (extended_config.parse_train_qkv): FP32Trainer's qkv."""
    from .extended_config import parse_train_qkv
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_qkv(hip)


def train_graph(cfg) -> bool:
    """cfg.hip.train_graph, checked (extended_config.parse_train_graph): `Learner.train_epoch` replays a captured step."""
    from .extended_config import parse_train_graph
    hip = cfg.get("hip", {}) if hasattr(cfg, "get") else {}
    return parse_train_graph(hip)


def averaged_weights_from_checkpoint(ck) -> Dict[str, torch.Tensor]:
    """A checkpoint's AVERAGED weights as a state dict: `averaging_state_dict`'s tensors over `model_state_dict` (a frozen
    parameter, and every parameter of a checkpoint saved before the first averaging update, is its own average). A checkpoint
    without the key was trained without cfg.hip.train_avg: a ValueError that says so."""
    asd = ck.get("averaging_state_dict")
    if asd is None:
        raise ValueError("cfg.hip.train_avg_eval: the checkpoint has no 'averaging_state_dict' (it was trained without "
                         "cfg.hip.train_avg), so there are no averaged weights to evaluate")
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in ck["model_state_dict"].items()}
    if int(asd["n_averaged"]) > 0:
        sd.update(asd["averaged"])
    return sd


class LRSchedule:
    """The reference's `prepare_scheduler` / `scheduler_step` (utils/trn_utils.py:806-823) without a torch optimizer to hang
    them on: torch's OWN scheduler classes run over a shell optimizer whose parameter groups mirror the given learning rates, so
    the sequence of rates is torch's, float for float. plateau = False: LambdaLR(lambda epoch: 1) (a constant rate);
    plateau = True: ReduceLROnPlateau(factor, patience) in torch's default mode ('min'), which is what the reference's call
    gets - on a metric where larger is better it cuts the rate while the metric improves. Needs no device."""

    def __init__(self, lrs, plateau: bool = False, factor: float = 0.1, patience: int = 10):
        self.plateau = bool(plateau)
        self.shell = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": float(lr)} for lr in lrs], lr=0.0)
        if self.plateau:
            self.sched = torch.optim.lr_scheduler.ReduceLROnPlateau(self.shell, factor=factor, patience=patience)
        else:
            self.sched = torch.optim.lr_scheduler.LambdaLR(self.shell, lambda epoch: 1)

    def lrs(self):
        return [float(g["lr"]) for g in self.shell.param_groups]

    def step(self, val_metric=None):
        """One epoch -> the learning rates from now on."""
        if self.plateau:
            self.sched.step(float(val_metric))
        else:
            self.shell.step()                                   # (no gradients: changes nothing; torch warns about a scheduler stepped first)
            self.sched.step()
        return self.lrs()

    def state_dict(self):
        return self.sched.state_dict()

    def load_state_dict(self, sd) -> None:
        """The scheduler's own state; the rates themselves are the optimizer's (restored with its state, as in torch)."""
        self.sched.load_state_dict(sd)


def params_opt_groups(mdl, params_opt_dict):
    """The reference's `params_opt_dict` (what `Learner.fit` hands to `opt_fn(params, lr=)`: an iterable of parameters, or
    torch parameter-group dicts) -> FP32Trainer's groups by NAME. Tensors are matched by identity through
    `mdl.named_parameters()`; names and prefixes pass through. A tensor that is not one of the model's is a ValueError.
    None -> None (every parameter, one learning rate)."""
    if params_opt_dict is None:
        return None
    by_id = {id(p): n for n, p in mdl.named_parameters()}

    def name_of(x, what):
        if isinstance(x, str):
            return x
        if not torch.is_tensor(x):
            raise ValueError(f"{what}: {type(x).__name__} is neither a parameter of the model nor a parameter name")
        if id(x) not in by_id:
            raise ValueError(f"{what}: a tensor of shape {tuple(x.shape)} is not one of the model's parameters")
        return by_id[id(x)]

    entries = list(params_opt_dict)
    if not all(isinstance(e, dict) for e in entries):
        if any(isinstance(e, dict) for e in entries):
            raise ValueError("params_opt_dict: either parameters or parameter-group dicts, not a mix")
        entries = [{"params": entries}]
    groups = []
    for gi, e in enumerate(entries):
        if "params" not in e:
            raise ValueError(f"params_opt_dict[{gi}]: no 'params'")
        ps = e["params"]
        ps = [ps] if (isinstance(ps, str) or torch.is_tensor(ps)) else list(ps)
        groups.append({**e, "params": [name_of(x, f"params_opt_dict[{gi}]") for x in ps]})
    return groups


def DataWrap(path, train_dl=None, valid_dl=None, test_dl=None):
    """utils/trn_utils.py:250-262."""
    return SimpleNamespace(path=Path(path), train_dl=train_dl, valid_dl=valid_dl, test_dl=test_dl)


class Learner:
    def __init__(self, uid: str, data, mdl, loss_fn, cfg, eval_fn, opt_fn=None, device=None, comm=None, train_mode: bool = True):
        self.uid, self.data, self.mdl, self.loss_fn, self.cfg, self.eval_fn = uid, data, mdl, loss_fn, cfg, eval_fn
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.rank = D.get_rank()
        self.comm = comm if comm is not None else getattr(mdl, "comm", None)
        self.loss_keys, self.met_keys = list(loss_fn.loss_keys), list(eval_fn.met_keys)
        self.log_keys = (["epochs"] + [f"trn_{k}" for k in self.loss_keys] + [f"val_{k}" for k in self.loss_keys]
                         + [f"val_{k}" for k in self.met_keys])
        self.init_log_dirs()
        self.num_it, self.num_epoch, self.best_met = 0, 0, 0.0
        opt = train_optimizer(cfg)
        avg = train_avg(cfg)
        self.avg_eval = avg["eval"]                             # validation (best_met, the plateau metric) on the averaged weights
        avg_kw = {} if avg["avg"] is None else dict(avg=avg["avg"], avg_decay=avg["decay"], avg_warmup=avg["warmup"],
                                                    avg_start=avg["start"], avg_every=avg["every"])
        self.lr_scheduler: Optional[LRSchedule] = None
        self._sched_state = None                                # a checkpoint's scheduler state, until `fit` builds the scheduler
        # dropout masks: independent across ranks and runs (the reference draws from torch's per-process generator)
        base_seed = int(torch.initial_seed()) & 0x7FFFFFFF
        self.trainer = FP32Trainer(cfg, self.comm, mdl.state_dict(), loss_fn, lr=float(cfg.train.lr), dropout=train_mode,
                                   dropout_seed=(base_seed * D.get_world_size() + self.rank) & 0x7FFFFFFF, amp=train_amp(cfg),
                                   loss_scale=train_loss_scale(cfg), clip_norm=train_clip_norm(cfg), freeze=train_freeze(cfg) or None,
                                   optimizer=opt["optimizer"], amsgrad=opt["amsgrad"], accum_steps=opt["accum_steps"], **avg_kw,
                                   **({"attn": train_attn(cfg)} if train_attn(cfg) != "materialized" else {}),
                                   **({"lstm": "fused"} if train_lstm(cfg) == "fused" else {}),
                                   **({"lstm_amp": "split"} if train_lstm_amp(cfg) == "split" else {}),
                                   **({"gemm_amp": "pipe"} if train_gemm_amp(cfg) == "pipe" else {}),
                                   **({"qkv": "factored"} if train_qkv(cfg) == "factored" else {}))
        # cfg.hip.train_graph: `train_epoch` replays a captured step (FP32Trainer.capture) for the batches of the epoch's shape.
        # What cannot be captured (accumulation windows, more than one rank) stays eager: the switch then changes nothing.
        from .train import capture_refusal
        self.train_graph = train_graph(cfg) and capture_refusal(opt["accum_steps"], D.get_world_size()) is None
        self.train_slot = None
        self.graph_replays, self.graph_fallbacks = 0, 0
        loaded_opt = False
        if cfg.train.resume:
            loaded_opt = bool(self.load_model_dict(resume_path=cfg.train.resume_path, load_opt=cfg.train.load_opt)) and bool(cfg.train.load_opt)
        # DistributedDataParallel broadcasts rank 0's parameters at construction: the replicas must not depend on seeding
        self.trainer.broadcast_from_rank0(with_optimizer=loaded_opt)
        if D.get_world_size() > 1:
            self._sync_model()

    # ---- files (init_log_dirs / create_log_dirs, utils/trn_utils.py:341-379)
    def init_log_dirs(self):
        p = Path(self.data.path)
        self.txt_log_file = p / "txt_logs" / f"{self.uid}.txt"
        self.model_file = p / "models" / f"{self.uid}.pth"
        self.predictions_dir = p / "predictions" / f"{self.uid}"
        if D.is_main_process():
            for d in (self.txt_log_file.parent, self.model_file.parent, self.predictions_dir):
                d.mkdir(parents=True, exist_ok=True)

    def update_log_file(self, towrite: str):
        if D.is_main_process():
            with self.txt_log_file.open("a") as f:
                f.write(towrite + "\n")

    @property
    def lr(self):
        return self.trainer.lr

    # ---- checkpoint (save_model_dict / load_model_dict, utils/trn_utils.py:533-630)
    def save_model_dict(self):
        if not D.is_main_process():
            return
        ck = {"model_state_dict": {k: v.cpu() for k, v in self.trainer.state_dict().items()},
              "optimizer_state_dict": self.trainer.optimizer_state_dict(), "num_it": self.trainer.num_it,
              "num_epoch": self.num_epoch, "cfgtxt": json.dumps(self.cfg, default=str), "best_met": self.best_met}
        ssd = self.trainer.scaler_state_dict()
        if ssd is not None:                                     # loss scaling on: torch.amp.GradScaler.state_dict()'s layout
            ck["scaler_state_dict"] = ssd
        asd = self.trainer.averaging_state_dict()
        if asd is not None:                                     # averaging on: model_state_dict stays the TRAINED parameters (a resume needs them)
            asd["averaged"] = {k: v.cpu() for k, v in asd["averaged"].items()}
            ck["averaging_state_dict"] = asd
        # the reference writes its scheduler's state into every checkpoint (utils/trn_utils.py:611-623); the constant schedule
        # has none worth keeping (LambdaLR's epoch count changes nothing), so the key appears with the plateau scheduler only
        if self.lr_scheduler is not None and self.lr_scheduler.plateau:
            ck["scheduler_state_dict"] = self.lr_scheduler.state_dict()
        torch.save(ck, self.model_file.open("wb"))

    def load_model_dict(self, resume_path: Optional[str] = None, load_opt: bool = False):
        mfile = self.model_file if not resume_path else Path(resume_path)
        if not mfile.exists():
            return False
        ck = torch.load(mfile.open("rb"), weights_only=False)
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in ck["model_state_dict"].items()}
        self.trainer.params.update({k: v.to(self.trainer.dev, torch.float32).contiguous() for k, v in sd.items()
                                    if k in self.trainer.params})
        if load_opt and "optimizer_state_dict" in ck:
            self.trainer.load_optimizer_state_dict(ck["optimizer_state_dict"])
        if load_opt and "scaler_state_dict" in ck:              # (a trainer without loss scale ignores it)
            self.trainer.load_scaler_state_dict(ck["scaler_state_dict"])
        if load_opt and "averaging_state_dict" in ck and self.trainer.avg_mode is not None:
            self.trainer.load_averaging_state_dict(ck["averaging_state_dict"])
        if load_opt and "scheduler_state_dict" in ck:           # (`prepare_scheduler` hands it to the scheduler it builds)
            self._sched_state = ck["scheduler_state_dict"]
        # the Learner's iteration counter is restored on every load (utils/trn_utils.py:588-590), with or without the
        # optimizer state: it also numbers the dropout masks, which must not restart. Adam's own step (bias correction) is
        # NOT touched here: without `load_opt` the reference builds a fresh Adam at step 0 (m = v = 0), and a step count of N
        # against zero moments would switch the bias correction off (first update ~3.2 x lr); `load_optimizer_state_dict`
        # restores it together with m / v.
        if "num_it" in ck:
            self.trainer.num_it = self.num_it = int(ck["num_it"])
        self.num_epoch, self.best_met = int(ck.get("num_epoch", 0)), float(ck.get("best_met", 0.0))
        self._sync_model()
        return True

    def _sync_model(self):
        """The trainer's parameters become the inference model's. cfg.hip.weight_refresh = device: they go to the engine as
        they are, on the device (`AnetBaseMdl.refresh_from_device`: weight images rewritten in place, captured slots and the
        evaluator's validation-graph pipeline stay valid); host (default): through `load_state_dict` and a full re-finalize.
        With cfg.hip.train_avg_eval the AVERAGED parameters go instead (`FP32Trainer.averaged_state_dict`: device tensors, no
        copies), so validation, best_met and the scheduler's metric are those of the averaged weights."""
        from .extended_config import parse_weight_refresh
        weights = self.trainer.averaged_state_dict() if self.avg_eval else self.trainer.params
        if parse_weight_refresh(self.cfg.get("hip", {})) == "device" and callable(getattr(self.mdl, "refresh_from_device", None)):
            self.mdl.refresh_from_device(weights)
            return
        self.mdl.load_state_dict({k: v.clone() for k, v in weights.items()} if self.avg_eval else self.trainer.state_dict(), strict=False)
        self.mdl.refresh_weights()

    # ---- learning-rate schedule (prepare_scheduler / scheduler_step, utils/trn_utils.py:806-823)
    def prepare_scheduler(self) -> LRSchedule:
        """The schedule over the trainer's learning rates as they are now (one per parameter group, then the trainer's own).
        Constant by default; with cfg.train.use_reduce_lr_plateau ReduceLROnPlateau on the first validation metric. The
        reference reads cfg.reduce_factor / cfg.patience, which no config defines: cfg.hip.train_plateau_factor /
        train_plateau_patience stand in for them. A scheduler state that came with a checkpoint (load_opt) is loaded once."""
        opt = train_optimizer(self.cfg)
        self.sched_using_val_metric = bool(self.cfg.train.get("use_reduce_lr_plateau", False))
        tr = self.trainer
        lrs = [tr.lr] if tr._groups is None else tr.group_lrs() + [tr.lr]
        sched = LRSchedule(lrs, self.sched_using_val_metric, opt["plateau_factor"], opt["plateau_patience"])
        if self._sched_state is not None and self.sched_using_val_metric:
            sched.load_state_dict(self._sched_state)
        self._sched_state = None
        return sched

    def scheduler_step(self, val_metric) -> None:
        """Once per epoch, after validation: the scheduler's rates become the trainer's and its groups'."""
        lrs = self.lr_scheduler.step(val_metric)
        self.trainer.set_lr(lrs[-1], None if self.trainer._groups is None else lrs[:-1])

    # ---- loops
    def _train_epoch_graph(self, sm) -> None:
        """The epoch's iterations with cfg.hip.train_graph: the first batch's shape is captured (or the slot of the previous
        epoch reused while it is not stale), every batch of that shape is one replay (`graph_replays`), any other shape - a
        short tail batch - the eager step (`graph_fallbacks`). The smoothed losses are fed in iteration order: a replay's
        values come from the slot's ring, read in one copy before a row could be overwritten and at the end of the epoch,
        where the slot's length guard is checked too."""
        tr = self.trainer
        pending = []                                            # per iteration since the last drain: None (a replay) | its loss dict

        def drain():
            slot = self.train_slot
            n = sum(1 for x in pending if x is None)
            rows = iter(slot.losses(n)) if n else iter(())
            for x in pending:
                sm.add_value(next(rows) if x is None else x)
            pending.clear()

        first_tick = None                                       # the oldest replay whose row is still unread
        for it, batch in enumerate(self.data.train_dl):
            batch = {k: v.to(tr.dev) for k, v in batch.items()}
            old = self.train_slot
            if old is None or (it == 0 and not old.matches(batch)) or (old.matches(batch) and old.stale_reason() is not None):
                if old is not None:
                    drain()
                    first_tick = None
                    old.release()
                self.train_slot = tr.capture(batch)
            slot = self.train_slot
            if slot.matches(batch):
                if first_tick is not None and tr.num_it - first_tick >= slot.log_rows:
                    drain()
                    first_tick = None
                first_tick = tr.num_it if first_tick is None else first_tick
                slot.step(batch)
                pending.append(None)
                self.graph_replays += 1
            else:
                pending.append(tr.step(batch))
                self.graph_fallbacks += 1
            self.num_it = tr.num_it
        if self.train_slot is not None:
            drain()
            self.train_slot.check()
        # (validation follows on its own graphs: nothing of the training graph is in flight behind this)
        torch.cuda.synchronize(tr.dev)

    def train_epoch(self, mb=None) -> Dict[str, float]:
        sm = SmoothenDict(self.loss_keys, 0.9)
        if self.train_graph:
            self._train_epoch_graph(sm)
        else:
            for batch in self.data.train_dl:
                batch = {k: v.to(self.trainer.dev) for k, v in batch.items()}
                sm.add_value(self.trainer.step(batch))
                self.num_it = self.trainer.num_it
        self.trainer.flush()                                    # (an accumulation window the epoch left open: applied with its own count)
        D.synchronize()
        out = dict(sm.smooth)
        if D.get_world_size() > 1:
            # reduce_dict(average=True) over the ranks (utils/trn_utils.py:61-90, 527-530)
            t = torch.tensor([float(out.get(k, 0.0)) for k in self.loss_keys], dtype=torch.float64, device=self.trainer.dev)
            torch.distributed.all_reduce(t)
            out = {k: float(v) / D.get_world_size() for k, v in zip(self.loss_keys, t.tolist())}
        return out

    def validate(self, db=None, mb=None, write_to_file: bool = False):
        if db is None:
            dl, dl_name = self.data.valid_dl, "valid"
        elif isinstance(db, dict):
            assert len(db) == 1
            dl_name, dl = next(iter(db.items()))
        else:
            dl, dl_name = db, "valid"
        self._sync_model()
        # a derived bank's rows (encodings, obj_tx rows, a `QueryLoader`'s argument vectors) belong to the weights they were made
        # with: after the sync they are the previous epoch's
        if callable(getattr(self.mdl, "engine", None)):
            for bank in (getattr(dl, "bank", None), getattr(dl, "queries", None)):
                if hasattr(bank, "stale") and bank.stale(self.mdl.engine()):
                    bank.refresh(engine=self.mdl.engine())
        with torch.no_grad():
            out_loss, out_acc = self.eval_fn(self.mdl, self.loss_fn, dl, dl_name, rank=self.rank, pred_path=self.predictions_dir)
        D.synchronize()
        if write_to_file:
            self.update_log_file("  ".join([f"val_{k} {float(out_loss[k]):.4f}" for k in self.loss_keys]
                                           + [f"val_{k} {float(out_acc[k]):.4f}" for k in self.met_keys]))
        return out_loss, out_acc, {}

    def testing(self, db):
        db = db if isinstance(db, dict) else {"dl0": db}
        res = {}
        for dl_name, dl in db.items():
            out_loss, out_acc, _ = self.validate({dl_name: dl}, write_to_file=True)
            res[dl_name] = (out_loss, out_acc)
        return res

    def fit(self, epochs: int, lr: Optional[float] = None, params_opt_dict=None, log=print):
        """`params_opt_dict` (the reference hands it to `opt_fn(params, lr=)`, utils/trn_utils.py:702-711): an iterable of the
        model's parameters (or names), or torch parameter-group dicts with their own `lr` / `weight_decay` - only these are
        trained, a group without `lr` at `lr`; None = every parameter (minus cfg.hip.train_freeze) at `lr`."""
        if lr is not None:
            self.trainer.lr = float(lr)
        self.trainer.set_param_groups(params_opt_groups(self.mdl, params_opt_dict))
        if self.train_slot is not None:                         # (captured for the previous groups)
            self.train_slot.release()
            self.train_slot = None
        self.lr_scheduler = self.prepare_scheduler()
        self.update_log_file("  ".join(self.log_keys) + "\n")
        hist, st, met = [], time.time(), None
        for _ in range(int(epochs)):
            self.num_epoch += 1
            trn = self.train_epoch()
            val_loss, val_acc, _ = self.validate(self.data.valid_dl)
            met = float(val_acc[self.met_keys[0]])
            self.scheduler_step(met)
            rec = {"epochs": self.num_epoch, **{f"trn_{k}": trn[k] for k in self.loss_keys},
                   **{f"val_{k}": float(val_loss[k]) for k in self.loss_keys}, **{f"val_{k}": float(val_acc[k]) for k in self.met_keys}}
            hist.append(rec)
            if self.best_met < met or not self.model_file.exists():
                self.best_met = max(self.best_met, met)
                self.save_model_dict()
            line = "  ".join(f"{v:.4f}" if isinstance(v, float) else str(v) for v in rec.values())
            self.update_log_file(line)
            if D.is_main_process():
                log("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in rec.items()))
            D.synchronize()
        self.update_log_file(f"epochs done {self.num_epoch}. Total time taken {time.time() - st: 0.4f}\n")
        return hist
