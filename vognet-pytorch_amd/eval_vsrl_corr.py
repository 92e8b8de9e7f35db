"""Prediction head of the "evaluator" on the plugin surface.

Same classes / ctor / `get_out_results_boxes` / record format as reference
code/eval_vsrl_corr.py (Evaluator{SEP,TEMP,SPAT}: 24-33, 162-424), with the
arg-max + box gather done by `vog_pred_head` on the GPU and the cross-rank
gather done by one RCCL all-gather (dist.py) instead of pickle files.
The validation loss comes from the device loss (`mdl_conc.LossB_*` -> `vog_loss_fwd`). Metrics: when the
annotation files of `cfg.ds` (`val_ds4_inds`, `anet_ent_annot_file`) exist, `after_init` builds the
`GroundEval_*` of the concatenation type (eval_fn_corr.py in this package, pinned against the reference's)
as the reference's `after_init` does (eval_vsrl_corr.py:154-158, 277-283, 349-351) and rank 0 scores the
merged pickle at the end of `forward`; without the files `val_acc` is zeros. With `cfg.hip.device_metrics` the records are
scored where they are produced (`vog_ground_metrics`, csrc/metrics.hip: one int32 of counts per record) and rank 0 only
aggregates those words; `cfg.hip.val_pickle = False` then drops the pickle and the record exchange that feeds it.
"""
from __future__ import annotations

import ctypes as C
import pickle
import time
from pathlib import Path

import numpy as np
import torch

from . import dist as D
from . import fast_pickle
from . import lib as L


def _as_bytes(t):
    """A bool mask travels as its bytes."""
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def gather_result_words(word_rows):
    """This rank's result words of vog_ground_metrics, one int32 [rows] tensor per ring entry (padding rows included) ->
    on rank 0 numpy [world, entries * rows], rank-major; None on the other ranks and without entries. Every rank holds
    the same number of entries (the metadata exchange of `Evaluator.forward` asserts it)."""
    if not word_rows:
        return None
    world = D.get_world_size()
    t = torch.stack(word_rows)                         # [entries, rows]
    if world > 1:
        outl = [torch.empty_like(t) for _ in range(world)]
        torch.distributed.all_gather(outl, t)
        t = torch.stack(outl)
    return t.cpu().numpy().reshape(world, -1) if D.is_main_process() else None


def merge_result_words(words_all, meta_all, meta_keys, meta_w):
    """(result words [world, n], per rank the metadata rows [..., W + 1] whose last column marks the real rows) -> (words,
    idx_sent) of the real rows in (rank, batch, row) order: the order of the records in the prediction pickle, which is the
    reference's merge order (code/eval_vsrl_corr.py:131-137) - so "the first record of a sentence wins" picks the same
    record on both paths, wrapped-around duplicates of a padded shard included."""
    off = 0
    for k in meta_keys:
        if k == "sent_idx":
            break
        off += meta_w[k]
    words, sents = [], []
    for r in range(len(meta_all)):
        mr = meta_all[r].reshape(-1, meta_all[r].shape[-1])
        assert mr.shape[0] == words_all[r].shape[0], (mr.shape, words_all[r].shape)
        keep = mr[:, -1] > 0
        words.append(words_all[r][keep])
        sents.append(mr[keep][:, off])
    return np.concatenate(words), np.concatenate(sents)


class Evaluator(torch.nn.Module):
    conc_type = None

    def __init__(self, cfg, comm, device):
        super().__init__()
        self.cfg = cfg
        self.comm = comm
        self.met_keys = ["avg1", "macro_avg1"]
        self.num_prop_per_frm = comm["num_prop_per_frm"]
        self.num_frms = cfg.ds.num_sampled_frm
        self.num_props = self.num_prop_per_frm * self.num_frms
        self.device = device
        self.grnd_eval = None
        self.after_init()

    def after_init(self):
        self.met_keys = ["avg1", "avg1_cons", "avg1_vidf", "avg1_strict"]
        self.num_sampled_frm = self.num_frms
        self.grnd_eval = self._make_grnd_eval()

    def _make_grnd_eval(self):
        import os
        from . import eval_fn_corr as M
        ds = self.cfg.ds
        files = [getattr(ds, k, None) if not isinstance(ds, dict) else ds.get(k) for k in ("val_ds4_inds", "anet_ent_annot_file")]
        if self.conc_type is None or not all(isinstance(f, str) and os.path.isfile(f) for f in files):
            return None
        cls = {"sep": M.GroundEval_SEP, "temp": M.GroundEval_TEMP, "spat": M.GroundEval_SPAT}[self.conc_type]
        return cls(self.cfg, self.comm)

    def _hip(self, key, default):
        hip = self.cfg.get("hip") if hasattr(self.cfg, "get") else getattr(self.cfg, "hip", None)
        if hip is None:
            return default
        return hip.get(key, default) if hasattr(hip, "get") else getattr(hip, key, default)

    # ---- device metrics --------------------------------------------------------
    def _ground_metrics(self, rec, batch, ncmp, nsrl, rows):
        """Result words of vog_ground_metrics for the records of one forward: int32 [rows] on the device (the rows past the
        batch stay zero = not scored), launched on the stream the records were produced on."""
        lib = L.load()
        nb = rec.shape[0]
        for k in ("sent_idx", "new_srl_idxs", "num_cmp_msk", "target_cmp"):
            if k not in batch:
                raise KeyError(f"cfg.hip.device_metrics needs batch['{k}']")
        cols = [batch[k].to(device=rec.device, dtype=torch.int64).contiguous() for k in ("sent_idx", "new_srl_idxs", "num_cmp_msk", "target_cmp")]
        assert cols[0].numel() == nb and cols[1].numel() == nb * ncmp and cols[2].numel() == nb * ncmp and cols[3].numel() == nb
        tab, _ = self.grnd_eval.device_table(rec.device)
        res = torch.zeros(rows, dtype=torch.int32, device=rec.device)
        a = L.GMetricArgs()
        a.rec = L.ptr(rec)
        a.idx_sent, a.idx_verbs, a.cmp_msk, a.targ_cmp = (L.ptr(c) for c in cols)
        a.tab = C.pointer(tab)
        a.result = L.ptr(res)
        a.B, a.ncmp, a.nsrl, a.nfrm0 = nb, ncmp, nsrl, self.num_frms
        a.conc_type = L.CONC_TYPE[self.conc_type]
        a.prob_thresh = float(self.grnd_eval.prob_thresh)
        L.check(lib.vog_ground_metrics(C.byref(a), L.stream_ptr()), "vog_ground_metrics")
        return res

    # ---- device head -----------------------------------------------------------
    def _records(self, out, inp):
        if "_pred_rec" in out:
            return out["_pred_rec"]
        lib = L.load()
        ev = out["mdl_outs_eval"].contiguous()
        B = ev.shape[0]
        ncmp = inp["new_srl_idxs"].size(1)
        nsrl = ev.shape[2]
        rb = int(lib.vog_pred_record_bytes(ncmp, nsrl, self.num_frms))
        rec = torch.empty(B, rb // 4, dtype=torch.float32, device=ev.device)
        a = L.PredArgs()
        a.outs_eval = L.ptr(ev)
        a.props = L.ptr(inp["pad_proposals"].contiguous())
        a.fin_scores = L.ptr(out["fin_scores"].contiguous()) if "fin_scores" in out else None
        a.rec = L.ptr(rec)
        a.B, a.ncmp, a.nsrl, a.nfrm0, a.nppf0 = B, ncmp, nsrl, self.num_frms, self.num_prop_per_frm
        a.conc_type = L.CONC_TYPE[self.conc_type]
        L.check(lib.vog_pred_head(C.byref(a), L.stream_ptr()), "vog_pred_head")
        return rec

    def unpack(self, rec, ncmp, nsrl):
        B = rec.shape[0]
        nb = nsrl * ncmp * self.num_frms
        boxes = rec[:, : nb * 7].reshape(B, nsrl, ncmp, self.num_frms, 7)
        scores = rec[:, nb * 7: nb * 8].reshape(B, nsrl, ncmp, self.num_frms)
        if self.conc_type == "temp":     # reference returns float zeros (eval_vsrl_corr.py:338-340)
            idx = torch.zeros(B, nsrl, self.num_frms, dtype=torch.float32, device=rec.device)
        else:
            idx = rec[:, nb * 8:].contiguous().view(torch.int64).reshape(B, nsrl, self.num_frms)
        return {"boxes": boxes, "scores": scores, "indexs": idx}

    def get_out_results_boxes(self, out_result_dict, inp):
        """-> {'boxes' [B,nsrl,ncmp,nfrm,7], 'scores' [B,nsrl,ncmp,nfrm], 'indexs' [B,nsrl,nfrm]}"""
        assert isinstance(out_result_dict, dict)
        rec = self._records(out_result_dict, inp)
        ncmp = inp["new_srl_idxs"].size(1)
        nsrl = out_result_dict["mdl_outs_eval"].shape[2]
        return self.unpack(rec, ncmp, nsrl)

    def forward_one_batch(self, out_result, inp):
        """Python-list records in the reference's format (eval_vsrl_corr.py:247-273)."""
        r = self.get_out_results_boxes(out_result, inp)
        cols = {
            "pred_boxes": r["boxes"], "pred_scores": r["scores"], "pred_cmp": r["indexs"],
            "idx_vid": inp["ann_idx"], "idx_verbs": inp["new_srl_idxs"], "idx_sent": inp["sent_idx"],
            "cmp_msk": inp["num_cmp_msk"], "targ_cmp": inp["target_cmp"], "perm": inp["permute"],
            "perm_inv": inp["permute_inv"],
        }
        cols = {k: v.detach().cpu().tolist() for k, v in cols.items()}
        n = len(cols["pred_boxes"])
        return [{k: v[i] for k, v in cols.items()} for i in range(n)]

    META_KEYS = ("ann_idx", "new_srl_idxs", "sent_idx", "num_cmp_msk", "target_cmp", "permute", "permute_inv")
    META_NAMES = {"ann_idx": "idx_vid", "new_srl_idxs": "idx_verbs", "sent_idx": "idx_sent", "num_cmp_msk": "cmp_msk",
                  "target_cmp": "targ_cmp", "permute": "perm", "permute_inv": "perm_inv"}
    GATHER_EVERY = 16          # batches per cross-rank exchange (dist.RecordRing half)

    def forward(self, model, loss_fn, dl, dl_name, rank=0, pred_path=None, mb=None):
        """The validation loop of the reference (code/eval_vsrl_corr.py:101-150): forward, loss_fn(out,
        batch), prediction records; rank 0 writes `<pred_path>/<dl_name>_<rank>.pkl` in the reference
        record format (:247-273) and returns (loss dict, metric dict).

        Exchange: the reference pickles per-rank predictions and rank 0 re-reads the files (:125-140).
        Here every batch's packed device records travel through ONE all-gather per GATHER_EVERY batches
        (dist.RecordRing; a collective per batch costs 12-20 us per step) and the batches' metadata (ids,
        masks, permutations: int64, known on the HOST before the batch is uploaded) stays on the host and
        is exchanged once, at the end. Record order on rank 0 = (rank, batch, query): all of rank 0's
        records, then all of rank 1's, ... - the order in which the reference appends the per-rank files
        (:131-137).

        Host side of the loop: the batches are uploaded `depth` batches ahead on a copy stream
        (dat_loader_simple.DevicePrefetcher) and the longest sentence is taken from the host copy of the
        lengths, so that no step of the loop waits for the device (the per-key blocking `.to(device)` and the
        `.item()` of the reference's loop cost 1.5 ms per cfg-2 batch)."""
        from .dat_loader_simple import DevicePrefetcher
        model.eval()
        world = D.get_world_size()
        # cfg.hip.device_metrics: score the records on the device (needs the annotations and records on a GPU; otherwise the
        # host pass over the pickle stays); cfg.hip.val_pickle = False: no pickle, hence no record exchange either
        dev_metrics = bool(self._hip("device_metrics", False)) and self.grnd_eval is not None and torch.device(self.device).type == "cuda"
        keep_pickle = bool(self._hip("val_pickle", True))
        if not keep_pickle and not dev_metrics:
            raise ValueError("cfg.hip.val_pickle = False leaves the metrics to the device path, which needs cfg.hip.device_metrics = True, "
                             "the annotation files of cfg.ds (val_ds4_inds, anet_ent_annot_file) and a GPU evaluator")
        self.metrics_path = "device" if dev_metrics else "host"
        word_rows = []                                 # this rank: per ring entry, int32 [rows_ring] result words (device)
        rec_rows = [[] for _ in range(world)]          # rank 0: per rank, the gathered record rows of every half (numpy)
        meta_rows = []                                 # this rank: per ring entry, int64 [rows_ring, W + 1] (last column: real row)
        losses = {}
        loss_log = []
        nums = 0
        ring = None
        layout = {}

        def check_faults():
            # (after a host synchronisation: every forward issued before it has completed) a stalled BiLSTM hand-off is an
            # error here, never NaN scores in the prediction pickle
            if hasattr(model, "check_faults"):
                model.check_faults()

        def on_half(g, n_valid):
            if not D.is_main_process():
                check_faults()
                return
            # ONE device-to-host copy of the gathered rows; everything else is host-side slicing
            host = g.view(world, self.GATHER_EVERY, layout["B"], -1)[:, :n_valid].detach().cpu().numpy()
            check_faults()
            for r in range(world):
                rec_rows[r].append(host[r].reshape(n_valid * layout["B"], -1))

        G = int(self.cfg.hip.get("batch_requests", 1)) if "hip" in self.cfg else 1
        dev = torch.device(self.device)
        # cfg.hip.val_graph: a validation step = one transfer + one graph launch (`_forward_graph`), where that loop can run
        self.val_path = "eager"
        from .extended_config import check_hip_options
        check_hip_options(self.cfg)                    # (cfg.hip.lang_bank without query_bank / val_graph is refused, not ignored)
        if bool(self._hip("val_graph", False)):
            if G > 1:
                raise ValueError("cfg.hip.val_graph serves one loader batch per forward: cfg.hip.batch_requests > 1 is not supported with it")
            eng, dl = self._graph_engine(model, loss_fn, dl, dev)
            if eng is None and bool(self._hip("lang_bank", False)):
                raise L.VogError("cfg.hip.lang_bank: this run cannot take the validation graph (the fp32 plan, whose language chain "
                                 "runs in fp32 from the word-level keys; a CPU evaluator; a loss that is not the device loss; a loader "
                                 "whose batches already live on the device) - switch it off")
            if eng is not None:
                self.val_path = "graph"
                return self._forward_graph(eng, model, loss_fn, dl, dl_name, rank, pred_path, dev, dev_metrics, keep_pickle)

        def host_T(bts):
            """Longest sentence of the group from the host copies of the lengths (None: they live on the device)."""
            ls = [bt.get("srl_arg_word_mask_len") for bt in bts]
            if any(l is None or l.is_cuda for l in ls):
                return None
            return max(int(l.max()) for l in ls)

        def batches():
            """(device batch, host batches, sizes): the loader's batches, `batch_requests` of them at a time as one
            (dynamic batching: rows never interact; concatenated on the device: 35 MB per group on the host cost 10 ms)."""
            pend, hosts = [], []
            for dbt, hbt in DevicePrefetcher(dl, dev, depth=2, hold=max(1, G)):
                if dev.type != "cuda" or not all(v.is_cuda for v in dbt.values()):
                    dbt = {k: v.to(dev) for k, v in dbt.items()}
                if G <= 1:
                    yield dbt, [hbt], [next(iter(dbt.values())).shape[0]]
                    continue
                pend.append(dbt)
                hosts.append(hbt)
                if len(pend) == G:
                    yield {k: torch.cat([p_[k] for p_ in pend], dim=0) for k in pend[0]}, hosts, [next(iter(p_.values())).shape[0] for p_ in pend]
                    pend, hosts = [], []
            if pend:
                yield {k: torch.cat([p_[k] for p_ in pend], dim=0) for k in pend[0]}, hosts, [next(iter(p_.values())).shape[0] for p_ in pend]

        for batch, hosts, sizes in batches():
            b = next(iter(batch.values())).shape[0]
            with torch.no_grad():
                T = host_T(hosts) if getattr(model, "supports_T_hint", False) else None
                out = model(batch, T=T) if T is not None else model(batch)
                if loss_fn is not None:
                    # the loss of every loader batch on its own rows: the reference averages per-batch means (:113-127)
                    lo = 0
                    for sz in sizes:
                        if len(sizes) == 1:
                            ld = loss_fn(out, batch)
                        else:
                            ld = loss_fn({k: v[lo:lo + sz] for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == b},
                                         {k: v[lo:lo + sz] for k, v in batch.items()})
                        # (kept as 0-dim device tensors and reduced ONCE behind the loop: a running `+= v.double() * sz` is three
                        # tiny launches per key and batch)
                        loss_log.append(({k: v.detach() for k, v in ld.items()}, sz))
                        nums += sz
                        lo += sz
            rec = self._records(out, batch)
            meta = [k for k in self.META_KEYS if k in batch]
            if not layout:
                # rows of one ring entry: the loader's batch size x the requests served per forward - not whatever this rank's
                # FIRST batch happens to hold (a wrapped-around shard can start with the short tail batch), and the same on
                # every rank (the all-gather's sizes must agree)
                rows_ring = max(rec.shape[0], int(self.cfg.train.get("bsv", 0) or 0) * max(1, G))
                if D.get_world_size() > 1:
                    t = torch.tensor([rows_ring], dtype=torch.int64, device=rec.device)
                    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
                    rows_ring = int(t.item())
                layout.update(B=rows_ring, rw=rec.shape[1], ncmp=batch["new_srl_idxs"].size(1),
                              nsrl=out["mdl_outs_eval"].shape[2], meta=meta,
                              meta_w={k: int(batch[k].numel() // rec.shape[0]) for k in meta},
                              meta_1d={k: batch[k].dim() == 1 for k in meta})
                if keep_pickle:
                    ring = D.RecordRing(rows_ring, rec.shape[1], self.GATHER_EVERY, rec.device, on_half=on_half)
            nb = rec.shape[0]
            assert nb <= layout["B"], (f"batch of {nb} queries, the exchange ring holds {layout['B']} per entry "
                                       "(cfg.train.bsv x cfg.hip.batch_requests, or the first batch if larger)")
            # metadata of the entry's rows from the HOST batches (a device-resident loader batch is read back: a sync per batch)
            m = np.zeros((layout["B"], sum(layout["meta_w"].values()) + 1), dtype=np.int64)
            lo = 0
            for hbt, sz in zip(hosts, sizes):
                off = 0
                for k in meta:
                    w = layout["meta_w"][k]
                    m[lo:lo + sz, off:off + w] = hbt[k].detach().cpu().numpy().reshape(sz, w)
                    off += w
                lo += sz
            m[:nb, -1] = 1                             # real rows: a short batch (validation loaders keep the tail,
            meta_rows.append(m)                        # drop_last=is_train, utils/trn_utils.py:200-203) is padded to the ring's rows
            if dev_metrics:
                if not rec.is_cuda:
                    raise ValueError("cfg.hip.device_metrics: the prediction records are not on a GPU")
                word_rows.append(self._ground_metrics(rec, batch, layout["ncmp"], layout["nsrl"], layout["B"]))
            if not keep_pickle:
                continue
            row = rec
            if nb < layout["B"]:
                row = torch.cat([rec, rec.new_zeros(layout["B"] - nb, rec.shape[1])], dim=0)
            ring.push(row, torch.cuda.current_stream() if rec.is_cuda else None)
        if ring is not None:
            ring.flush()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        check_faults()
        if loss_log:
            wts = torch.tensor([float(sz) for _, sz in loss_log], dtype=torch.float64, device=next(iter(loss_log[0][0].values())).device)
            for k in loss_log[0][0]:
                losses[k] = (torch.stack([d[k] for d, _ in loss_log]).double() * wts).sum()

        def rec_fn():
            return [np.concatenate(rec_rows[r], axis=0) if rec_rows[r] else np.zeros((0, layout["rw"]), np.float32) for r in range(world)]

        return self._finish(dev, layout, meta_rows, rec_fn, losses, nums, lambda: gather_result_words(word_rows), dev_metrics,
                            keep_pickle, pred_path, dl_name, rank)

    # ---- cfg.hip.val_graph ------------------------------------------------------------------------------
    VAL_GRAPH_GEOMETRY = (4, 2)        # forward streams x fed slots per stream (tests set it on the instance)

    def _graph_engine(self, model, loss_fn, dl, dev):
        """(the engine `_forward_graph` runs on, the loader) - the engine is None where the existing loop has to serve: a CPU
        evaluator, a model that does not expose its engine, the fp32 plan (its eager forward overwrites a slot's outputs
        behind the graph, so a graph's epilogue would read the 16-bit ones), a loss that is not the device loss
        (`mdl_conc.LossB_*`: the epilogue calls vog_loss_fwd with its settings), a loader without a length or whose batches
        already live on the device. A loader that is neither a list nor a `BankLoader` (a torch DataLoader) is read ONCE
        into a list here - the setup scans every host batch for the longest sentence and the modal shape, so the epoch's
        host batches are held in memory - and that list is what either loop then runs on."""
        from .dat_loader_simple import BankLoader
        if dev.type != "cuda" or not callable(getattr(model, "engine", None)):
            return None, dl
        if loss_fn is not None and not hasattr(loss_fn, "_forward_values"):
            return None, dl
        try:
            len(dl)
        except TypeError:
            return None, dl
        eng = model.engine()
        if eng.device != dev or eng.precise is not None:
            return None, dl
        if not isinstance(dl, BankLoader):
            if not isinstance(dl, (list, tuple)):
                dl = list(dl)
            if any(isinstance(v, torch.Tensor) and v.is_cuda for bt in dl for v in bt.values()):
                return None, dl
        return eng, dl

    def _forward_graph(self, eng, model, loss_fn, dl, dl_name, rank, pred_path, dev, dev_metrics, keep_pickle):
        """`forward` with every full-shape batch served by a fed slot whose graph ends in the validation epilogue
        (engine.FedPipeline(..., epilogue=)): per batch the host writes the batch and its step number into the next staging
        buffer and submits; loss, result words and records land in row `step` of the device logs (engine.ValLog) and are
        read once behind the loop. Batches of another shape (the short tail) take the eager calls and write their row with
        a stand-alone vog_val_log. Same loss expression, record order and pickle bytes as the loop above.
        cfg.hip.query_bank: the host batches' per-query rows live in a `dat_loader_simple.QueryBank` (built once per loader)
        and the host writes `qry_index` and `val_step` per step; the slots' graphs gather the rows (`_query_bank`).
        cfg.hip.lang_bank (with query_bank): the word-level columns of that bank are replaced by the language chain's results at
        (B, T_max) of this pass under the engine's current weights (`_lang_bank`: a `dat_loader_simple.LangBank`, re-encoded
        when `weights_epoch` or the plan moved); the slots are vector-form, their forwards start behind the BiLSTM, and a batch
        of another shape takes the eager vector form with its rows gathered by the bank."""
        from .dat_loader_simple import BANK_KEYS, PER_QUERY_KEYS, BankLoader
        from .engine import ARG_KEYS, F32_KEYS, NSRL_KEYS_I64, WORD_KEYS, Epilogue
        from .extended_config import check_hip_options
        check_hip_options(self.cfg)
        world = D.get_world_size()
        bank = dl.bank if isinstance(dl, BankLoader) else None
        hosts = [{k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in bt.items()}
                 for bt in (dl.index_loader if bank is not None else dl)]
        n_steps = len(hosts)
        sep = eng.sep
        # what the device reads: the forward's keys, the loss keys, the metric columns - everything else (ids, permutations,
        # tags) stays on the host. A bank produces the visual and ground-truth keys from `vid_index` and the per-query keys.
        want = list(NSRL_KEYS_I64 + F32_KEYS) + (["verb_ind_in_srl"] if sep else [])
        if loss_fn is not None:
            want += [k for k, _ in Epilogue.LOSS_KEYS + (Epilogue.SEP_KEYS if sep else ())]
        if dev_metrics:
            want += list(Epilogue.METRIC_KEYS)
        want = list(dict.fromkeys(want))
        if bank is not None:
            produced = set(BANK_KEYS) | {"pad_frm_mask"}
            staged = ["vid_index"] + [k for k in PER_QUERY_KEYS] + [k for k in want if k not in produced and k not in PER_QUERY_KEYS]
        else:
            staged = want

        def sig(bt):
            return tuple((k, tuple(bt[k].shape), _as_bytes(bt[k]).dtype) for k in staged)

        sigs = [sig(bt) for bt in hosts]
        modal = max(set(sigs), key=lambda g: (sigs.count(g), -sigs.index(g))) if sigs else None
        T_max = max([int(bt["srl_arg_word_mask_len"].max()) for bt in hosts], default=1)
        B = int(hosts[sigs.index(modal)]["srl_arg_words_ind"].shape[0]) if sigs else 1
        ncmp = int(hosts[0]["new_srl_idxs"].size(1)) if hosts else 1
        rw = eng.record_words(ncmp)
        layout = {}
        meta_rows = []
        nums = 0
        wts = []
        pipe, log, qb, gathered = None, None, None, []
        lbk, arg_ex = None, {}
        if hosts:
            first = hosts[sigs.index(modal)]
            meta = [k for k in self.META_KEYS if k in first]
            layout.update(B=B, rw=rw, ncmp=ncmp, nsrl=int(eng.desc.nsrl), meta=meta,
                          meta_w={k: int(first[k].numel() // B) for k in meta}, meta_1d={k: first[k].dim() == 1 for k in meta})
            if bool(self._hip("query_bank", False)):
                # the per-video arrays of a host loader's batches (what a feature bank would hold) stay staged: the query bank
                # holds the per-query part only
                heavy = set(BANK_KEYS) | {"pad_frm_mask"}
                gathered = [k for k in staged if k not in heavy]
                qb = self._query_bank(dl, hosts, gathered, dev)
                staged = [k for k in staged if k in heavy]
                meta_mat, row0 = self._val_graph_cache["qbank"][2:4]
                if bool(self._hip("lang_bank", False)):
                    lbk = self._lang_bank(eng, qb, B, T_max)
                    arg_keys = [k for k in ARG_KEYS if k in lbk.tab]
                    gathered = [k for k in gathered if k not in WORD_KEYS] + arg_keys
                    with torch.cuda.device(dev):
                        arg_ex = {k: torch.zeros((B,) + lbk.spec[k][0], dtype=torch.float32, device=dev) for k in arg_keys}
            pipe, log = self._graph_pipeline(eng, bank, first, staged, modal, T_max, n_steps, B, rw if keep_pickle else 0,
                                             loss_fn, dev_metrics, lbk if lbk is not None else qb, gathered, arg_ex)
        use_T = getattr(model, "supports_T_hint", False)
        t_loop = time.perf_counter()
        for step, (hb, g) in enumerate(zip(hosts, sigs)):
            nb = int(hb["srl_arg_words_ind"].shape[0])
            assert nb <= B, f"batch of {nb} queries, the validation log holds {B} per step"
            m = np.zeros((B, sum(layout["meta_w"].values()) + 1), dtype=np.int64)
            if qb is not None:                          # the host columns of the query bank: one slice, no device
                m[:nb, :-1] = meta_mat[row0[step]:row0[step] + nb]
            else:
                off = 0
                for k in layout["meta"]:
                    w = layout["meta_w"][k]
                    m[:nb, off:off + w] = hb[k].numpy().reshape(nb, w)
                    off += w
            m[:nb, -1] = 1
            meta_rows.append(m)
            if loss_fn is not None:
                wts.append(float(nb))
                nums += nb
            if g == modal:
                st = pipe.next_staging()
                if qb is not None:
                    torch.arange(int(row0[step]), int(row0[step]) + B, dtype=torch.int32, out=st.host["qry_index"])
                for k in staged:
                    st.host[k].copy_(_as_bytes(hb[k]))
                st.host["val_step"][0] = step
                pipe.submit()
                continue
            # another shape: the eager calls on the current stream, behind the pipeline's work so far; its own row of the logs
            cur = torch.cuda.current_stream(dev)
            for fs in pipe.streams:
                cur.wait_stream(fs)
            with torch.no_grad():
                if bank is not None:
                    batch = next(iter(BankLoader(bank, [hb])))
                else:
                    batch = {k: v.to(dev, non_blocking=True) for k, v in hb.items()}
                if lbk is not None:                     # the eager vector form: this batch's rows of the language bank
                    rows = lbk(torch.arange(int(row0[step]), int(row0[step]) + nb, dtype=torch.int32), keys=list(arg_ex))
                    rows.pop("_keepalive", None)
                    batch = {**{k: v for k, v in batch.items() if k not in WORD_KEYS}, **rows}
                T = int(hb["srl_arg_word_mask_len"].max()) if use_T else None
                out = model(batch, T=T) if T is not None else model(batch)
                loss_src = None
                if loss_fn is not None:
                    ld = loss_fn(out, batch)
                    vals = [ld["loss"], ld["mdl_out_loss"]] + ([ld["verb_loss"]] if "verb_loss" in ld else [])
                    loss_src = torch.cat([torch.stack([v.detach() for v in vals]), torch.zeros(6 - len(vals), device=dev)])
                rec = self._records(out, batch)
                words = self._ground_metrics(rec, batch, ncmp, layout["nsrl"], B) if dev_metrics else None
                rec_src = None
                if keep_pickle:
                    rec_src = rec if nb == B else torch.cat([rec, rec.new_zeros(B - nb, rec.shape[1])], dim=0)
                log.write(step, loss_src, words, rec_src, stream=cur)
        t_host = time.perf_counter() - t_loop           # the host's share: filling the staging buffers and submitting
        torch.cuda.synchronize()
        self.val_graph_stats = {"steps": n_steps, "host_s": t_host, "graph_steps": sum(g == modal for g in sigs),
                                "staging_bytes": pipe.stagings[0].nbytes if pipe is not None else 0,
                                "query_bank_bytes": qb.nbytes if qb is not None else 0,
                                "lang_bank_bytes": lbk.nbytes if lbk is not None else 0,
                                "lang_encode_seconds": lbk.encode_seconds if lbk is not None else 0.0}
        if hasattr(model, "check_faults"):
            model.check_faults()
        if pipe is not None:
            for sl in pipe.slots:
                sl.check()                              # stalled hand-offs, bank indices, the step guard
            log.check()
            log.check_written(n_steps)
        losses = {}
        if loss_fn is not None and n_steps:
            w = torch.tensor(wts, dtype=torch.float64, device=dev)
            for i, k in enumerate(["loss", "mdl_out_loss"] + (["verb_loss"] if sep else [])):
                losses[k] = (log.loss[:n_steps, i].double() * w).sum()

        def exchange(t):
            """This rank's rows of a log -> rank 0: numpy [world, ...], rank-major; ONE exchange and one device-to-host copy."""
            if world > 1:
                outl = [torch.empty_like(t) for _ in range(world)]
                torch.distributed.all_gather(outl, t)
                t = torch.stack(outl)
            else:
                t = t[None]
            return t.cpu().numpy() if D.is_main_process() else None

        if world > 1:                                   # (the all-gathers' sizes must agree: steps and rows per step)
            cnt = torch.tensor([n_steps, -n_steps, B, -B], dtype=torch.int64, device=dev)
            torch.distributed.all_reduce(cnt, op=torch.distributed.ReduceOp.MAX)
            assert int(cnt[0]) == -int(cnt[1]), "every rank must run the same number of validation batches (DistributedSampler pads)"
            assert int(cnt[2]) == -int(cnt[3]), "every rank must run the same validation batch size"
        rec_all = None
        if keep_pickle and n_steps:
            rec_all = exchange(log.rec[:n_steps].contiguous())

        def rec_fn():
            return [rec_all[r].reshape(n_steps * B, rw) for r in range(world)]

        def words_fn():
            if not n_steps:
                return None
            wa = exchange(log.words[:n_steps].contiguous())
            return wa.reshape(world, -1) if wa is not None else None

        return self._finish(dev, layout, meta_rows, rec_fn, losses, nums, words_fn, dev_metrics, keep_pickle, pred_path, dl_name, rank)

    def _query_bank(self, dl, hosts, staged, dev):
        """The `QueryBank` of this loader's host batches (`staged`: the keys the device reads, `vid_index` of a bank loader's
        index batches among them), built once per loader object - cached by the loader's identity and length, whatever
        happens to the engine's weights - with the metadata columns as one host matrix [Q, W] in the order of META_KEYS and
        the first row of every step."""
        from .dat_loader_simple import QueryBank
        cache = self.__dict__.setdefault("_val_graph_cache", {})
        hit = cache.get("qbank")
        key = (id(dl), len(hosts), tuple(staged), str(dev))
        if hit is not None and hit[0] == key and hit[4] is dl:
            return hit[1]
        cache.pop("qbank", None)
        meta = [k for k in self.META_KEYS if k in hosts[0]]
        cols = list(dict.fromkeys(list(staged) + meta))
        with torch.cuda.device(dev):
            qb = QueryBank.from_batches([{k: _as_bytes(bt[k]) for k in cols} for bt in hosts], keys=cols, host_keys=meta, device=dev)
        sizes = [int(bt[staged[0]].shape[0]) for bt in hosts]
        row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        rows = qb.meta(np.arange(qb.Q))
        meta_mat = (np.concatenate([rows[k].reshape(qb.Q, -1).astype(np.int64) for k in meta], axis=1) if meta
                    else np.zeros((qb.Q, 0), np.int64))
        cache["qbank"] = (key, qb, meta_mat, row0, dl)          # (holds the loader: its id cannot be reused meanwhile)
        return qb

    def _lang_bank(self, eng, qb, B, T_max):
        """The `LangBank` of `qb` for this engine at (B, T_max), kept in `_val_graph_cache` while the query bank and the geometry
        stay; its rows belong to the engine's `weights_epoch` and plan - when either moved since they were encoded
        (`Learner.validate` after a training epoch) they are re-encoded in place: the tables keep their addresses."""
        from .dat_loader_simple import LangBank
        cache = self.__dict__.setdefault("_val_graph_cache", {})
        key = (id(qb), id(eng), int(B), int(T_max))
        hit = cache.get("lbank")
        if hit is not None and hit[0] == key and hit[2] is qb:
            lbk = hit[1]
            if lbk.stale(eng):
                lbk.refresh(engine=eng)
            return lbk
        cache.pop("lbank", None)
        cache.pop("pipe", None)                         # (its slots gather from the old bank's tables)
        lbk = LangBank.encode(qb, eng, int(B), int(T_max))
        cache["lbank"] = (key, lbk, qb)
        return lbk

    def _graph_pipeline(self, eng, bank, first, staged, modal, T_max, n_steps, B, rec_words, loss_fn, dev_metrics, qb=None, gathered=(),
                        arg_ex=None):
        """The fed pipeline and its logs for this shape, built once and kept while the engine's weight buffers stay (a reload
        moves `layout_epoch`: with cfg.hip.weight_refresh = host `Learner.validate` reloads every epoch and old slots refuse to
        launch; with "device" the weights are rewritten in place and the pipeline lives on) and the logs are large enough.
        `arg_ex`: example tensors of the keys among `gathered` that the host batches do not hold (a language bank's columns)."""
        arg_ex = arg_ex or {}
        from .engine import Epilogue, FedPipeline, ValLog
        streams, per = self.VAL_GRAPH_GEOMETRY
        key = (id(eng), eng.layout_epoch, id(bank), modal, T_max, rec_words, loss_fn is not None and id(loss_fn), dev_metrics,
               int(streams), int(per), id(qb))
        cache = self.__dict__.setdefault("_val_graph_cache", {})
        hit = cache.get("pipe")
        if hit is not None and hit[0] == key and hit[2].rows >= n_steps:
            pipe, log = hit[1], hit[2]
            for t in (log.loss, log.words, log.rec, log.written):
                if t is not None:
                    t.zero_()
            cur = torch.cuda.current_stream(eng.device)
            for fs in pipe.streams:                     # the first log launch of this run comes behind the clearing
                fs.wait_stream(cur)
            return pipe, log
        hit = None
        cache.pop("pipe", None)                         # (frees the old slots before the new ones are allocated)
        dev = eng.device

        with torch.cuda.device(dev):
            log = ValLog(dev, n_steps, B, loss=loss_fn is not None, words=dev_metrics, rec_words=rec_words)
            epi = Epilogue(log, loss_fn=loss_fn, grnd_eval=self.grnd_eval if dev_metrics else None)
            # with a query bank the host writes B + 1 integers per step: the rows' numbers and the step
            spec = {k: _as_bytes(first[k]) for k in staged}
            if qb is not None:
                spec["qry_index"] = torch.zeros(B, dtype=torch.int32)
            spec["val_step"] = torch.zeros(4, dtype=torch.int32)
            if bank is not None:
                per_query = {k: first[k].to(dev) for k in ("target_cmp", "srl_boxes", "srl_boxes_lens") if k in first}
                ex = bank(first["vid_index"], per_query, with_loss_keys=False)
                ex.pop("_keepalive", None)
                ex.update({k: (arg_ex[k] if k in arg_ex else _as_bytes(first[k])) for k in list(staged) + list(gathered) if k != "vid_index"})
            else:
                ex = {k: (arg_ex[k] if k in arg_ex else _as_bytes(first[k])) for k in list(staged) + list(gathered)}
            pipe = FedPipeline(eng, ex, spec, assembler=bank, streams=int(streams), slots_per_stream=int(per), T=T_max,
                               with_pred=True, epilogue=epi, queries=qb)
        cache["pipe"] = (key, pipe, log)
        return pipe, log

    def _finish(self, dev, layout, meta_rows, rec_fn, losses, nums, words_fn, dev_metrics, keep_pickle, pred_path, dl_name, rank):
        """Behind the loop, after its one synchronisation (both loops end here): the metadata exchange, the pickle, the loss
        means and the metrics. `rec_fn()` -> on rank 0, per rank, the record rows [entries * rows_ring, rw] (numpy);
        `words_fn()` -> on rank 0 the result words [world, entries * rows_ring]; `losses`: per key the size-weighted sum."""
        world = D.get_world_size()
        # the metadata of every rank on rank 0: one exchange for the whole loop
        meta_all = None
        if meta_rows:
            mine = np.stack(meta_rows)                 # [entries, rows_ring, W + 1]
            if world > 1:
                t = torch.from_numpy(mine).to(dev)
                cnt = torch.tensor([t.shape[0], -t.shape[0]], dtype=torch.int64, device=dev)
                torch.distributed.all_reduce(cnt, op=torch.distributed.ReduceOp.MAX)
                assert int(cnt[0]) == -int(cnt[1]), "every rank must run the same number of validation batches (DistributedSampler pads)"
                outl = [torch.empty_like(t) for _ in range(world)]
                torch.distributed.all_gather(outl, t)
                meta_all = [o.cpu().numpy() for o in outl] if D.is_main_process() else None
            else:
                meta_all = [mine]
        # kept as numpy columns; the reference's per-query dicts of Python lists (eval_vsrl_corr.py:247-273) are never
        # built: rank 0 writes their pickle bytes directly (fast_pickle.dumps_records, byte-identical;
        # `tolist` + `pickle.dumps` of 512 queries cost 170 ms = a 3 k queries/s ceiling for the whole validation loop)
        chunks = []                                    # (rank, batch) order: the reference's merge order
        if D.is_main_process() and meta_all is not None and keep_pickle:
            rec_all = rec_fn()
            for r in range(world):
                rows = rec_all[r]
                mr = meta_all[r].reshape(-1, meta_all[r].shape[-1])
                assert rows.shape[0] == mr.shape[0], (rows.shape, mr.shape)
                keep = mr[:, -1] > 0
                u = self.unpack(torch.from_numpy(np.ascontiguousarray(rows[keep])), layout["ncmp"], layout["nsrl"])
                cols = {"pred_boxes": u["boxes"].numpy(), "pred_scores": u["scores"].numpy(), "pred_cmp": u["indexs"].numpy()}
                off = 0
                for k in layout["meta"]:
                    w = layout["meta_w"][k]
                    mk = mr[keep][:, off:off + w]
                    cols[self.META_NAMES[k]] = np.ascontiguousarray(mk[:, 0] if layout["meta_1d"][k] else mk)
                    off += w
                chunks.append(cols)
        merged = {k: np.concatenate([c[k] for c in chunks], axis=0) for k in chunks[0]} if chunks else {}
        val_loss = {k: (v / max(1, nums)).float() for k, v in losses.items()}
        if D.get_world_size() > 1:
            for k in sorted(val_loss):                 # as reduce_dict in the reference (utils/trn_utils.py:61-90)
                t = val_loss[k].clone()
                torch.distributed.all_reduce(t)
                val_loss[k] = t / world
        val_acc = {k: torch.tensor(0.0) for k in self.met_keys}
        # the result words of every rank on rank 0: 4 bytes per record, one exchange and ONE device-to-host copy
        words_all = words_fn() if dev_metrics else None
        if D.is_main_process() and pred_path is not None and keep_pickle:
            fname = Path(pred_path) / f"{dl_name}_{rank}.pkl"
            fname.parent.mkdir(parents=True, exist_ok=True)
            with open(fname, "wb") as f:
                f.write(fast_pickle.dumps_records(merged) if merged else pickle.dumps([]))
            if self.grnd_eval is not None and not dev_metrics:
                acc = self.grnd_eval.eval_ground_acc(fname)
                val_acc = {k: torch.tensor(v) for k, v in acc.items() if k in self.met_keys}
        if D.is_main_process() and dev_metrics:
            # (rank, batch, row) order = the order of the pickle's records: "first record of a sentence wins" picks the same one
            words, sents = np.zeros(0, np.int32), np.zeros(0, np.int64)
            if words_all is not None:
                words, sents = merge_result_words(words_all, meta_all, layout["meta"], layout["meta_w"])
            acc = self.grnd_eval.eval_ground_acc_from_results(words, sents)
            val_acc = {k: torch.tensor(v) for k, v in acc.items() if k in self.met_keys}
        D.synchronize()
        return val_loss, val_acc


class EvaluatorSEP(Evaluator):
    conc_type = "sep"


class EvaluatorTEMP(Evaluator):
    conc_type = "temp"


class EvaluatorSPAT(Evaluator):
    conc_type = "spat"
