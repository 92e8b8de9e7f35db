"""CLI with the reference's shape (code/main_dist.py:90-163):

    python -m vognet_amd.main_dist <uid> [--dotted.cfg.key=value ...] [--local_rank=N]

`fire` is not installed, so the `uid --a.b=c` syntax is parsed here; overrides go
through `update_from_dict` (unknown key / type mismatch -> AssertionError, as
code/extended_config.py:69-78). `--only_val=True` / `--only_test=True` run the reference's validation flow
(code/main_dist.py:143-157 -> `Learner.validate`, utils/trn_utils.py:443-468): the selected evaluator is
called as `eval_fn(mdl, loss_fn, dl, dl_name, rank=..., pred_path=<tmp_path>/predictions/<uid>)`, i.e.
forward -> device loss -> prediction records -> ONE cross-rank exchange per 16 batches (dist.RecordRing) ->
rank 0 writes `<pred_path>/<dl_name>_0.pkl` and scores it when the annotation files of cfg.ds exist; the
loss and metric dicts are printed like the reference prints them, followed by one JSON line.
Without `only_val` / `only_test` it builds `trn_utils.Learner` and runs `learn.fit` (code/main_dist.py:31-87, 125 ->
utils/trn_utils.py:701-775): per epoch the device training step (`train.FP32Trainer`: fp32 forward -> loss -> backward -> gradient
all-reduce -> Adam) over the training batches, then the validation flow above on the inference model carrying the
new weights, and `<tmp_path>/models/<uid>.pth` in the reference's checkpoint layout; `--train.resume=True` loads
it back (model + optimizer), as `Learner.load_model_dict`.
The dataset readers are out of scope: without the 530 GB dataset the loaders are lists of
synthetic batches (`--synthetic_batches=N`, the last validation batch a query short like the tail batch of a
`drop_last=False` loader). `--feature_bank=f16` (or `f32`; `--feature_bank_videos=N`, default 256) keeps the synthetic
video segments in a device-resident `dat_loader_simple.FeatureBank` and runs both flows on index batches.
`--feature_bank=enc` validates / tests from a `dat_loader_simple.EncodedBank` (the encoder outputs of the videos under the
loaded weights, encoded once from an f16 bank); in `fit` the raw f16 bank feeds training and the encoded one, refreshed
after every epoch's weight sync, feeds validation.
`--feature_bank=obj` does the same from a `dat_loader_simple.ObjBank` (obj_tx's output rows: the forward starts at mul_tx) -
sep / svsq models with an object transformer only.
`--query_bank=True` (needs `--feature_bank`) also keeps the synthetic per-query keys on the device, in a
`dat_loader_simple.QueryBank`, and runs both flows on `{qry_index, vid_index}` batches.
`--query_bank=lang` does the same with the validation / test queries in a `dat_loader_simple.LangBank` (the language chain's
results under the loaded weights, encoded once from the query bank at the validation batch size and the loader's longest
sentence; `lang_encode_seconds` in the JSON line): those forwards start behind the BiLSTM. In `fit` the plain query bank feeds
training and the language bank, refreshed after every epoch's weight sync, feeds validation.
`--hip.train_freeze=enc,lang` (stages of engine.TRAIN_STAGES: lang, enc, obj) trains the rest only (`FP32Trainer(freeze=)`): the
frozen stages get no gradient and no Adam state. The training loaders stay the raw ones (raw bank, plain query bank) also with
a frozen stage; the JSON line of a `fit` run names the frozen stages (`train_freeze`).
`--hip.train_optimizer=adamw` (decoupled weight decay; default `adam`), `--hip.train_amsgrad=True` and
`--hip.train_accum_steps=N` (N micro-batches per optimiser step; an epoch's last, shorter window is applied with its own count)
select the optimiser variant of the training step (`FP32Trainer(optimizer=, amsgrad=, accum_steps=)`).
`--train.use_reduce_lr_plateau=True` steps torch's ReduceLROnPlateau on the first validation metric once per epoch, with
`--hip.train_plateau_factor` (0.1) and `--hip.train_plateau_patience` (10); the JSON line of a `fit` run reports the final `lr`.
`--hip.train_attn=fused` runs the encoder layers' attention of the training step through the fused operator (`vog_attn_fused_f32`:
O(N) scratch, three launches for all heads; `FP32Trainer(attn=)`); the default `materialized` is the step as it always was.
`--hip.train_attn=fused_pipe` runs that operator on its pipelined kernels (two LDS buffers, one barrier per staged tile): the
bits and the scratch of `fused`.
`--hip.train_lstm=fused` runs the fp32 BiLSTM recurrence of the training step in one launch per layer and step (`FP32Trainer(lstm=)`).
`--hip.train_lstm_amp=split` runs the recurrence under `--hip.train_amp` in the kernels that split K over the waves of a workgroup
(`FP32Trainer(lstm_amp=)`; the default `tile` keeps the wave-per-gate kernels, and without `train_amp` the key changes nothing).
`--hip.train_gemm_amp=pipe` runs the vector tile products under `--hip.train_amp` in the pipelined 16-bit tile kernel
(`FP32Trainer(gemm_amp=)`; the same bits as the default `tile`, and without `train_amp` the key changes nothing).
`--hip.train_qkv=factored` computes the Q / K / V projections of mul_tx's first layer from the two factors of its tokens - the
obj_tx row of the proposal and the masked argument vector - instead of from every `[vis | lang]` token, and sums dQ / dK / dV back
to the factors before the gradient products (`FP32Trainer(qkv=)`; `vog_attn_f32_vl` / `vog_attn_fused_f32_vl`). It combines with
every `train_attn`, `train_amp`, `train_gemm_amp` and `train_freeze` value, changes the order of the fp32 sums (not the same bits
as the default `dense`), and does nothing for a model without mul_tx.
`--hip.train_avg=ema` (or `swa`; `--hip.train_avg_decay`, `train_avg_warmup`, `train_avg_start`, `train_avg_every`) keeps an average
of the parameters on the device behind every applied optimiser step (`FP32Trainer(avg=)`); the checkpoint then carries
`averaging_state_dict` beside the trained `model_state_dict`. With `--hip.train_avg_eval=True` a `fit` run validates on the averaged
weights, and `--only_val=True --hip.train_avg=ema --hip.train_avg_eval=True` evaluates the averaged weights of the checkpoint
(`--train.resume_path`, default `<tmp_path>/models/<uid>.pth`); a checkpoint without the key is an error that says so.
`--hip.train_graph=True` captures the training iteration once per epoch shape - forward, loss, backward, optimiser, averaging - and
replays it with one graph launch per batch (`FP32Trainer.capture`, `TrainSlot`); a batch of another shape (a short tail batch) runs
the eager step. Off by default; with `train_accum_steps` > 1 or more than one rank the epochs stay eager. The option changes more
than the launch count: a replay runs the language side over T = the width of the word mask where the eager step runs it over the
batch's longest sentence. Without dropout that moves no bit; a `fit` run trains with dropout, whose mask indices on the language
side depend on T, so its losses and weights are those of other (equally distributed) masks than the eager run's.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path
from typing import Any, Dict, List, Tuple

import torch

from . import dist as D
from . import synth
from .extended_config import (get_default_cfg, key_maps, num_prop_per_frm, post_proc_config,
                              update_from_dict)
from .mdl_selector import get_mdl_loss_eval


def parse_argv(argv: List[str]) -> Tuple[str, Dict[str, Any]]:
    if not argv or argv[0].startswith("--"):
        raise SystemExit("usage: main_dist.py <uid> [--a.b.c=value ...]")
    uid, kw = argv[0], {}
    i = 1
    while i < len(argv):
        a = argv[i]
        if not a.startswith("--"):
            raise SystemExit(f"unexpected argument {a!r}")
        if "=" in a:
            k, v = a[2:].split("=", 1)
        else:
            k = a[2:]
            if i + 1 < len(argv) and not argv[i + 1].startswith("--"):
                v = argv[i + 1]
                i += 1
            else:
                v = "True"
        kw[k] = v
        i += 1
    return uid, kw


def learner_init(uid: str, cfg):
    """Builds comm -> model / loss / eval like reference main_dist.py:31-87 (the data side and the trainer
    replaced by the synthetic loader below)."""
    sel = get_mdl_loss_eval(cfg)
    comm = {"vocab_size": 5000, "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1},
            "num_prop_per_frm": num_prop_per_frm(cfg)}
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    loss_fn = sel["loss"](cfg, comm)
    device = torch.device("cuda", torch.cuda.current_device())
    evl = sel["eval"](cfg, comm, device)
    return mdl, loss_fn, evl, comm


def synthetic_loader(cfg, comm, n_batches: int, rank: int, world: int, train: bool = False, pin: bool = True):
    """Validation batches with every key the forward, the loss and the evaluator read,
    this rank's contiguous share (dist.shard_indices = NewDistributedSampler, utils/trn_utils.py:127-156);
    the last batch is one query short (validation loaders keep the tail, trn_utils.py:200-203)."""
    import numpy as np
    bs = int(cfg.train.bs if train else cfg.train.bsv)
    ct = cfg.ds.conc_type
    out = []
    idx = list(D.shard_indices(n_batches, rank, world))
    if not train and (n_batches - 1) in idx:
        # shard_indices wraps around: the one short batch may not be the first a rank sees (a loader yields its tail last)
        idx = [i for i in idx if i != n_batches - 1] + [n_batches - 1] * idx.count(n_batches - 1)
    for i in idx:
        b = synth.make_batch(ct, bs, comm["num_prop_per_frm"], vocab_size=comm["vocab_size"], seed=1000 * i + (500000 if train else 0))
        b.update(synth.make_targets(b, ct, comm["num_prop_per_frm"], seed=i))
        ncmp = b["num_cmp_msk"].shape[1]
        rng = np.random.default_rng(77 + i)
        perm = np.stack([rng.permutation(ncmp) for _ in range(bs)]).astype(np.int64)
        b.update({"ann_idx": np.arange(i * bs, (i + 1) * bs, dtype=np.int64),
                  "sent_idx": np.arange(i * bs, (i + 1) * bs, dtype=np.int64),
                  "permute": perm, "permute_inv": np.argsort(perm, axis=1).astype(np.int64)})
        if i == n_batches - 1 and bs > 1 and not train:
            b = {k: v[: bs - 1] for k, v in b.items()}
        t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()}
        if pin and torch.cuda.is_available():
            # what DataLoader(pin_memory=True) hands over: the evaluator's `.to(device, non_blocking=True)` is then an
            # asynchronous copy at link speed (pageable tensors go through the runtime's bounce buffers: ~15 GB/s, 67 ms
            # of the 134 ms a 128-batch validation loop took)
            t = {k: v.pin_memory() for k, v in t.items()}
        out.append(t)
    return out


def synthetic_bank(cfg, comm, n_videos: int, dtype: str, chunk: int = 64):
    """A `dat_loader_simple.FeatureBank` of `n_videos` synthetic video segments (synth.make_items, one video per item),
    filled chunk by chunk: what a run on the dataset builds once from `simple_item_getter` items."""
    from .dat_loader_simple import BANK_KEYS, FeatureBank
    bank = FeatureBank(cfg, comm, n_videos, dtype=dtype)
    for s0 in range(0, n_videos, chunk):
        n = min(chunk, n_videos - s0)
        it = synth.make_items(n, 1, comm["num_prop_per_frm"], prop_dim=bank.prop_dim, seg_dim=bank.seg_dim, n_gt=bank.G,
                              seed=7919 + s0)
        bank.put(s0, {k: it[k][:, 0] for k in BANK_KEYS})
    return bank


def synthetic_index_loader(cfg, comm, n_batches: int, rank: int, world: int, n_videos: int, train: bool = False):
    """`synthetic_loader`'s batches with the visual and ground-truth keys replaced by `vid_index` [B, ncmp] (rows of the bank,
    uniformly random) and the per-query keys of synth.make_items: the language and mask keys of synth.make_batch, the
    evaluator's ids - a few KB per batch."""
    import numpy as np
    bs = int(cfg.train.bs if train else cfg.train.bsv)
    ct = cfg.ds.conc_type
    out = []
    idx = list(D.shard_indices(n_batches, rank, world))
    if not train and (n_batches - 1) in idx:
        idx = [i for i in idx if i != n_batches - 1] + [n_batches - 1] * idx.count(n_batches - 1)
    for i in idx:
        b = synth.make_batch(ct, bs, 1, vocab_size=comm["vocab_size"], prop_dim=4, seg_dim=4, seed=1000 * i + (500000 if train else 0))
        for k in ("pad_region_feature", "seg_feature_for_frms", "pad_proposals"):
            del b[k]
        ncmp = b["num_cmp_msk"].shape[1]
        it = synth.make_items(bs, ncmp, 1, prop_dim=4, seg_dim=4, n_gt=4, seed=i)
        rng = np.random.default_rng(77 + i)
        perm = np.stack([rng.permutation(ncmp) for _ in range(bs)]).astype(np.int64)
        b.update({k: it[k] for k in ("target_cmp", "srl_boxes", "srl_boxes_lens")})
        if ct in ("sep", "svsq"):                     # LossB_SEP's verb keys
            b.update({"verb_cmp": (rng.uniform(size=(bs, ncmp)) < 0.5).astype(np.int64),
                      "verb_cross_cmp_msk": (rng.uniform(size=(bs, ncmp, ncmp)) < 0.6).astype(np.int64)})
        b.update({"vid_index": rng.integers(0, n_videos, size=(bs, ncmp)).astype(np.int32),
                  "srl_arg_boxes_mask": (b["srl_arg_inds_msk"] * (rng.uniform(size=b["srl_arg_inds_msk"].shape) < 0.8)).astype(np.int64),
                  "ann_idx": np.arange(i * bs, (i + 1) * bs, dtype=np.int64),
                  "sent_idx": np.arange(i * bs, (i + 1) * bs, dtype=np.int64),
                  "permute": perm, "permute_inv": np.argsort(perm, axis=1).astype(np.int64)})
        if i == n_batches - 1 and bs > 1 and not train:
            b = {k: v[: bs - 1] for k, v in b.items()}
        out.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()})
    return out


def query_bank_loader(index_dl, bank, lang_engine=None, lang_B=None):
    """The index batches' per-query keys in a `dat_loader_simple.QueryBank` (built once), the loader reduced to
    `{qry_index, vid_index}` batches: `QueryBank.loader` gathers the rows and runs the feature bank's assembly behind them.
    `lang_engine`: the bank becomes a `LangBank` encoded on that engine at (`lang_B`, the longest sentence of the loader)."""
    from .dat_loader_simple import LangBank, QueryBank
    qb = QueryBank.from_batches(index_dl, keys=[k for k in index_dl[0] if k != "vid_index"], device=bank.device)
    if lang_engine is not None:
        T = max(int(bt["srl_arg_word_mask_len"].max()) for bt in index_dl)
        qb = LangBank.encode(qb, lang_engine, int(lang_B), T)
    small, row = [], 0
    for bt in index_dl:
        n = int(bt["vid_index"].shape[0])
        small.append({"qry_index": torch.arange(row, row + n, dtype=torch.int32), "vid_index": bt["vid_index"]})
        row += n
    return qb.loader(small, bank)


def main_dist(uid: str, **kwargs):
    cfg = get_default_cfg()
    cfg.uid = uid
    cfg.cmd = list(sys.argv)
    n_batches = int(kwargs.pop("synthetic_batches", 20))
    bank_dtype = kwargs.pop("feature_bank", None)             # "f32" | "f16": batches are assembled on the device from a bank
    bank_videos = int(kwargs.pop("feature_bank_videos", 256))
    qb_arg = str(kwargs.pop("query_bank", "False")).lower()
    if qb_arg not in ("true", "1", "false", "0", "lang"):
        raise SystemExit(f"--query_bank={qb_arg}: one of True, False, lang")
    query_bank, lang_bank = qb_arg in ("true", "1", "lang"), qb_arg == "lang"
    if query_bank and not bank_dtype:
        raise SystemExit(f"--query_bank={'lang' if lang_bank else 'True'} needs --feature_bank=f16 | f32 | enc | obj (its batches are "
                         "{qry_index, vid_index})")
    if "local_rank" in kwargs:
        cfg.do_dist = True
        torch.cuda.set_device(int(kwargs["local_rank"]))
        D.init_from_env("nccl")
        D.synchronize()
    cfg.num_gpus = torch.cuda.device_count()
    cfg = update_from_dict(cfg, kwargs, key_maps)
    cfg = post_proc_config(cfg)
    cfg.freeze()
    averaged = None
    if (cfg.only_val or cfg.only_test) and bool(cfg.hip.get("train_avg_eval", False)):
        # evaluate the checkpoint's AVERAGED weights (cfg.train.resume_path, or where `fit` writes <tmp_path>/models/<uid>.pth);
        # read before the model is built: a checkpoint without averages is refused at once
        from .trn_utils import averaged_weights_from_checkpoint
        mfile = Path(cfg.train.resume_path) if cfg.train.resume_path else Path(cfg.misc.tmp_path) / "models" / f"{uid}.pth"
        if not mfile.exists():
            raise SystemExit(f"--hip.train_avg_eval=True: no checkpoint at {mfile} (set --train.resume_path)")
        averaged = averaged_weights_from_checkpoint(torch.load(mfile.open("rb"), weights_only=False))
    if bank_dtype == "obj":
        from .engine import OBJ_MODEL_RULE
        has_obj = cfg.mdl.name == "vgrnd" or (cfg.mdl.name == "vog" and bool(cfg.mdl.obj_tx.to_use))
        if cfg.ds.conc_type not in ("sep", "svsq") or not has_obj:
            raise SystemExit(f"--feature_bank=obj ({cfg.mdl.name}, {cfg.ds.conc_type}): {OBJ_MODEL_RULE}")
    mdl, loss_fn, evl, comm = learner_init(uid, cfg)
    rank, world = D.get_rank(), D.get_world_size()
    # Learner.init_log_dirs (utils/trn_utils.py:341-368): <data.path = cfg.misc.tmp_path>/predictions/<uid>
    pred_path = Path(cfg.misc.tmp_path) / "predictions" / uid
    if bank_dtype not in (None, "f32", "f16", "enc", "obj"):
        raise SystemExit(f"--feature_bank={bank_dtype}: one of f16, f32, enc, obj")
    encoded = bank_dtype in ("enc", "obj")
    bank = synthetic_bank(cfg, comm, bank_videos, "f16" if encoded else str(bank_dtype)) if bank_dtype else None

    def encoded_bank():
        """The encoded counterpart of `bank` under the model's current weights, for the validation batch shape."""
        from .dat_loader_simple import EncodedBank, ObjBank
        from .lib import VogError
        ncmp = 1 if cfg.ds.conc_type == "svsq" else 4          # (videos per query of the synthetic batches)
        try:
            return (ObjBank if bank_dtype == "obj" else EncodedBank).encode(bank, mdl.engine(), int(cfg.train.bsv), ncmp)
        except (ValueError, VogError) as e:
            if bank_dtype != "obj":
                raise
            raise SystemExit(f"--feature_bank=obj: {e}")
    if not (cfg.only_val or cfg.only_test):
        # learner_init + learn.fit (code/main_dist.py:31-87, 125)
        from .trn_utils import DataWrap, Learner
        if bank is not None:
            mk = (lambda idl: query_bank_loader(idl, bank)) if query_bank else bank.loader
            # training reads raw features and the word-level keys, whatever cfg.hip.train_freeze says: the trainer takes a derived
            # bank's rows for a stage that is frozen whole (FP32Trainer), but these loaders do not feed it from one yet;
            # validation may start behind the encoders / the language side
            vbank = encoded_bank() if encoded else bank
            mkv = ((lambda idl: query_bank_loader(idl, vbank, mdl.engine() if lang_bank else None, int(cfg.train.bsv)))
                   if query_bank else vbank.loader)
            data = DataWrap(path=cfg.misc.tmp_path,
                            train_dl=mk(synthetic_index_loader(cfg, comm, n_batches, rank, world, bank.V, train=True)),
                            valid_dl=mkv(synthetic_index_loader(cfg, comm, max(2, n_batches // 2), rank, world, bank.V)))
        else:
            data = DataWrap(path=cfg.misc.tmp_path, train_dl=synthetic_loader(cfg, comm, n_batches, rank, world, train=True),
                            valid_dl=synthetic_loader(cfg, comm, max(2, n_batches // 2), rank, world))
        learn = Learner(uid=uid, data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)
        t0 = time.time()
        hist = learn.fit(epochs=int(cfg.train.epochs), lr=float(cfg.train.lr))
        torch.cuda.synchronize()
        if D.is_main_process():
            print(json.dumps({"uid": uid, "world": world, "epochs": len(hist), "train_steps": learn.trainer.num_it,
                              "seconds": time.time() - t0, "model_file": str(learn.model_file),
                              "train_freeze": sorted(learn.trainer.frozen_stages()), "lr": learn.trainer.lr,
                              "history": hist}))
        return hist
    dl_name = "valid" if cfg.only_val else "test"
    if averaged is not None:
        mdl.load_state_dict(averaged, strict=False)
    if bank is not None:
        if encoded:
            bank = encoded_bank()
        index_dl = synthetic_index_loader(cfg, comm, n_batches, rank, world, bank.V)
        dl = (query_bank_loader(index_dl, bank, mdl.engine() if lang_bank else None, int(cfg.train.bsv)) if query_bank
              else bank.loader(index_dl))
        nq_local = sum(int(b["num_cmp_msk"].shape[0]) for b in index_dl)
    else:
        dl = synthetic_loader(cfg, comm, n_batches, rank, world)
        nq_local = sum(int(b["num_cmp_msk"].shape[0]) for b in dl)
    if hasattr(mdl, "engine"):
        mdl.engine()                                  # register the weights (once per model, 0.6 s) outside the timed loop
    torch.cuda.synchronize()
    t0 = time.time()
    with torch.no_grad():
        val_loss, val_acc = evl(mdl, loss_fn, dl, dl_name, rank=rank, pred_path=pred_path)
    torch.cuda.synchronize()
    dt = time.time() - t0
    if D.is_main_process():
        print(val_loss)                               # as the reference (main_dist.py:147-148)
        print(val_acc)
        fname = pred_path / f"{dl_name}_0.pkl"
        print(json.dumps({"uid": uid, "world": world, "queries": nq_local * world, "seconds": dt,
                          "queries_per_s": nq_local * world / dt, "mdl": cfg.mdl.name,
                          "conc_type": cfg.ds.conc_type, "dl_name": dl_name, "pred_file": str(fname),
                          "metrics": getattr(evl, "metrics_path", "host"), "val_path": getattr(evl, "val_path", "eager"),
                          "feature_bank": bank_dtype, "query_bank": "lang" if lang_bank else query_bank,
                          "lang_encode_seconds": float(dl.queries.encode_seconds) if lang_bank else 0.0,
                          "val_loss": {k: float(v) for k, v in val_loss.items()},
                          "val_acc": {k: float(v) for k, v in val_acc.items()}}))
    return val_loss, val_acc


if __name__ == "__main__":
    _uid, _kw = parse_argv(sys.argv[1:])
    main_dist(_uid, **_kw)
