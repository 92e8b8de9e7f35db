"""Device-side SPAT / TEMP batch assembly — the step in front of the forward path.

The reference builds a SPAT / TEMP sample on the CPU inside the dataset
(`AV_CS.verb_item_getter_SPAT / _TEMP`, code/dat_loader_simple.py:1046-1338): four per-video items are
shifted (x += 720 * video / frame += 10 * video), re-ordered and concatenated, one query at a time, and
the collated batch is copied to the GPU. Here the per-video items of a whole batch (what
`AV_CS.itemcollector` stacks, [B, ncmp, ...]) are handed over as they are and `vog_assemble_batch`
(csrc/assemble.hip) writes the forward's / loss's tensors straight into their device buffers - e.g. a
`Slot`'s persistent inputs. Dataset reading itself (h5 / csv files, the 530 GB dataset) stays out of scope.
`FeatureBank` keeps the per-video items of a whole dataset on the device and assembles from video indices; `QueryBank`
keeps the per-query arrays there and gathers them from query indices (`vog_gather_rows`).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import lib as L
from .engine import ARG_KEYS, ENC_KEYS, LANG_KEYS, OBJ_KEYS, OBJ_MODEL_RULE, WORD_KEYS

FWD_KEYS = ("pad_proposals", "pad_region_feature", "seg_feature_for_frms")


class PackedStaging:
    """Host -> device staging of a batch as ONE copy. The tensors of a batch (per-video items for the assembler, word-level
    language arrays, ...) live back to back, 256-byte aligned, in ONE pinned host buffer and in one device buffer of the same
    layout; `host[k]` / `dev[k]` are views. `upload()` is a single asynchronous H2D copy of the used bytes on the current
    stream (13 per-key `copy_` calls measured 8.9 GB/s on the driver's box in round 3: every call pays its own launch and
    its own sub-MB transfer; the link wants one large one). The loader side fills `host[k]` in place (`fill`, or writes
    straight into the views), so nothing is concatenated on the host."""

    def __init__(self, spec: Dict[str, torch.Tensor], device: Optional[torch.device] = None, n_dev: int = 1):
        """spec: name -> example tensor / array (shape and dtype are taken from it; its values are copied in).
        n_dev = 2: two device buffers used alternately (`upload` flips), so that the copy of batch i + 1 - issued on a
        copy stream - runs while the forward of batch i still reads its own (`upload_on`)."""
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        ex = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in spec.items()}
        self.layout, off = {}, 0
        for k, v in ex.items():
            nb = v.numel() * v.element_size()
            self.layout[k] = (off, nb, tuple(v.shape), v.dtype)
            off += (nb + 255) // 256 * 256
        self.nbytes = off
        self.hbuf = torch.empty(off, dtype=torch.uint8).pin_memory()
        self.dbufs = [torch.empty(off, dtype=torch.uint8, device=self.device) for _ in range(max(1, int(n_dev)))]
        self.host = {k: self.hbuf[o:o + nb].view(dt).view(*shp) for k, (o, nb, shp, dt) in self.layout.items()}
        self.devs = [{k: b[o:o + nb].view(dt).view(*shp) for k, (o, nb, shp, dt) in self.layout.items()} for b in self.dbufs]
        self.dbuf, self.dev = self.dbufs[0], self.devs[0]
        self._cur = 0
        self._ready = [None] * len(self.dbufs)       # event: the copy into buffer b has landed
        self._free = [None] * len(self.dbufs)        # event: the consumer of buffer b is done reading it
        self.fill(ex)

    def fill(self, items: Dict[str, torch.Tensor]) -> "PackedStaging":
        for k, v in items.items():
            if k in self.host:
                self.host[k].copy_(v if isinstance(v, torch.Tensor) else torch.from_numpy(v))
        return self

    def upload(self) -> Dict[str, torch.Tensor]:
        """ONE async copy on the current stream; returns the device views (valid once the stream reaches this point)."""
        b = self._cur
        self._cur = (b + 1) % len(self.dbufs)
        self.dbufs[b].copy_(self.hbuf, non_blocking=True)
        return self.devs[b]

    def upload_on(self, copy_stream: "torch.cuda.Stream", consumer: Optional["torch.cuda.Stream"] = None):
        """The same copy on `copy_stream` (so it overlaps whatever the consumer stream is still running - a copy issued on
        the forward's own stream waits for the previous forward there: 11.5 k instead of 26 k queries/s at cfg 2), into the
        next device buffer. The consumer stream (default: the current one) waits for the copy; call `release()` on it once
        the kernels that read the views are enqueued, so the buffer's next copy waits for them. Returns the device views."""
        b = self._cur
        self._cur = (b + 1) % len(self.dbufs)
        cons = consumer if consumer is not None else torch.cuda.current_stream(self.device)
        if self._free[b] is not None:
            copy_stream.wait_event(self._free[b])
        with torch.cuda.stream(copy_stream):
            self.dbufs[b].copy_(self.hbuf, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        self._ready[b] = ev
        cons.wait_event(ev)
        self._last = b
        return self.devs[b]

    def release(self, consumer: Optional["torch.cuda.Stream"] = None) -> None:
        cons = consumer if consumer is not None else torch.cuda.current_stream(self.device)
        ev = torch.cuda.Event()
        ev.record(cons)
        self._free[self._last] = ev


class DevicePrefetcher:
    """`for dev_batch, host_batch in DevicePrefetcher(loader, device, depth, hold)`: the loader's batches (dicts of CPU tensors)
    as device batches whose host -> device copies were issued `depth` batches ahead on a copy stream, so that they overlap the
    forwards of the batches in front of them and the loop never waits for a copy it has just issued (the reference's
    `batch[k].to(device)` per key and batch, code/utils/trn_utils.py:478 / :562, is a blocking copy per key: 1.2 ms per
    cfg-2 batch, 6 forwards' worth).

    The copies land in persistent device buffers (a ring of depth + hold + 1 sets per batch shape; a batch of another shape -
    the short tail batch - gets a set of its own); a set is rewritten only after the consumer's stream has passed the point
    where it gave the batch back: the consumer may keep using the last `hold` batches it was handed (dynamic batching
    concatenates `hold` of them), nothing older. Batches that already live on the device pass through untouched.
    Pinned host tensors make the copies asynchronous; pageable ones still work (staged by the runtime)."""

    def __init__(self, loader, device, depth: int = 2, hold: int = 1):
        self.loader, self.device = loader, torch.device(device)
        self.depth, self.hold = max(1, int(depth)), max(1, int(hold))

    def __iter__(self):
        dev = self.device
        if dev.type != "cuda":
            for bt in self.loader:
                yield bt, bt
            return
        from collections import deque
        cs = torch.cuda.Stream(device=dev)
        nring = self.depth + self.hold + 1
        ring: list = [None] * nring
        given = {}                                   # batch number -> event on the consumer's stream behind its use
        pending = deque()
        n = 0

        SMALL = 64 << 10        # tensors below this travel together: one pinned buffer, ONE transfer (a transfer costs ~8 us of
                                # copy-engine time whatever its size: 20 KB-sized arrays per batch were 40 % of a cfg-2 batch's copies)

        def make_set(bt, sig):
            small = [k for k, v in bt.items() if v.numel() * v.element_size() < SMALL]
            e = {"sig": sig, "bufs": {k: torch.empty(v.shape, dtype=v.dtype, device=dev) for k, v in bt.items() if k not in small},
                 "small": small}
            if small:
                off, lay = 0, {}
                for k in small:
                    v = bt[k]
                    nb = v.numel() * v.element_size()
                    lay[k] = (off, nb)
                    off += (nb + 255) // 256 * 256
                e["hpack"] = [torch.empty(off, dtype=torch.uint8).pin_memory() for _ in range(2)]     # filled alternately:
                e["hfree"] = [None, None]                                                             # a buffer is rewritten once its transfer is done
                e["dpack"] = torch.empty(off, dtype=torch.uint8, device=dev)
                e["hviews"] = [{k: h[o:o + nb].view(bt[k].dtype).view(bt[k].shape) for k, (o, nb) in lay.items()} for h in e["hpack"]]
                for k, (o, nb) in lay.items():
                    e["bufs"][k] = e["dpack"][o:o + nb].view(bt[k].dtype).view(bt[k].shape)
                e["turn"] = 0
            e["bufs"] = {k: e["bufs"][k] for k in bt}           # the loader's key order
            return e

        def issue(bt):
            nonlocal n
            if any(v.is_cuda for v in bt.values()):
                pending.append((bt, bt, None))
                n += 1
                return
            sig = tuple((k, tuple(v.shape), v.dtype) for k, v in bt.items())
            e = ring[n % nring]
            cur = torch.cuda.current_stream(dev)
            if e is None or e["sig"] != sig:
                # new buffers come from the consumer stream's pool: whatever used that memory before is ordered on that stream
                e = make_set(bt, sig)
                ring[n % nring] = e
                ev = torch.cuda.Event()
                ev.record(cur)
                cs.wait_event(ev)
            else:
                m = n - nring + self.hold - 1          # the batch whose hand-back frees this set
                if m in given:
                    cs.wait_event(given[m])
            small = e["small"]
            if small:
                t = e["turn"]
                e["turn"] = 1 - t
                if e["hfree"][t] is not None:
                    e["hfree"][t].synchronize()        # (two uses of this set ago: long done)
                hv = e["hviews"][t]
                for k in small:
                    hv[k].copy_(bt[k])
            with torch.cuda.stream(cs):
                for k, v in bt.items():
                    if not small or k not in hv:
                        e["bufs"][k].copy_(v, non_blocking=True)
                if small:
                    e["dpack"].copy_(e["hpack"][t], non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(cs)
                if small:
                    e["hfree"][t] = ready
            pending.append((e["bufs"], bt, ready))
            n += 1

        def hand_out():
            dbt, hbt, ready = pending.popleft()
            if ready is not None:
                torch.cuda.current_stream(dev).wait_event(ready)
            return dbt, hbt

        j = 0
        for bt in self.loader:
            issue(bt)
            if len(pending) > self.depth:
                yield hand_out()
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                given[j] = ev
                given.pop(j - 2 * nring, None)
                j += 1
        while pending:
            yield hand_out()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            given[j] = ev
            j += 1


class DeviceBatchAssembler:
    def __init__(self, cfg, comm):
        self.conc_type = cfg.ds.conc_type
        assert self.conc_type in ("spat", "temp"), "sep / svsq batches need no assembly (verb_item_getter_SEP)"
        self.nfrm0 = int(cfg.ds.num_sampled_frm)
        self.nppf0 = int(comm["num_prop_per_frm"])
        self.vid_w = float(cfg.ds.resized_width)
        self.lib = L.load()

    def __call__(self, items: Dict[str, torch.Tensor], out: Optional[Dict[str, torch.Tensor]] = None,
                 with_loss_keys: bool = True) -> Dict[str, torch.Tensor]:
        a, out = self.args(items, out, with_loss_keys)
        L.check(self.lib.vog_assemble_batch(C.byref(a), L.stream_ptr()), "vog_assemble_batch")
        return out

    def args(self, items: Dict[str, torch.Tensor], out: Optional[Dict[str, torch.Tensor]] = None,
             with_loss_keys: bool = True):
        """The vog_assemble_args of this call and the destination dict, without launching (a fed slot captures the launch
        into its graph: `engine.Slot.feed_from`).
        items: device tensors with leading axes [B, ncmp] - or PINNED host tensors (zero copy: pinned memory is mapped
        into the device's address space, the kernels read it over the host link, so the batch needs no DMA of its own and
        none of a copy's fixed latency; `out` must then name the destination tensors, which also fixes the device).
        `out`: optional existing destination tensors (e.g. `slot.inp`) for any of the produced keys; missing ones are
        allocated."""
        P = items["pad_proposals"]
        assert (P.is_cuda or P.is_pinned()) and P.dtype == torch.float32 and P.dim() == 4 and P.shape[-1] == 7
        B, ncmp, NPv, _ = P.shape
        assert NPv == self.nfrm0 * self.nppf0
        if P.is_cuda:
            dev = P.device
        else:
            assert out and "pad_region_feature" in out, "pinned host items: pass the destination tensors in `out`"
            dev = out["pad_region_feature"].device
            assert all(items[k].is_pinned() for k in ("pad_region_feature", "seg_feature_for_frms")), "host items must be pinned"
        R, S = items["pad_region_feature"], items["seg_feature_for_frms"]
        out = dict(out or {})

        def dst(k, shape, dtype):
            t = out.get(k)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
                out[k] = t
            assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_cuda and t.is_contiguous(), k
            return t

        a = L.AssembleArgs()
        keep = [P.contiguous(), R.contiguous(), S.contiguous()]
        a.props_in, a.region_in, a.seg_in = (L.ptr(t) for t in keep)
        a.props_out = L.ptr(dst("pad_proposals", (B, ncmp * NPv, 7), torch.float32))
        a.region_out = L.ptr(dst("pad_region_feature", (B, ncmp * NPv, R.shape[-1]), torch.float32))
        a.seg_out = L.ptr(dst("seg_feature_for_frms", (B, ncmp * self.nfrm0, S.shape[-1]), torch.float32))
        if "pad_pnt_mask" in items:
            pm = items["pad_pnt_mask"].to(torch.uint8).contiguous()
            keep.append(pm)
            a.pnt_in, a.pnt_out = L.ptr(pm), L.ptr(dst("pad_pnt_mask", (B, ncmp * NPv), torch.uint8))
        if with_loss_keys and "pad_gt_bboxs" in items:
            G = items["pad_gt_bboxs"].shape[2]
            sb = items["srl_boxes"]
            for k in ("pad_gt_bboxs", "num_box", "target_cmp", "srl_boxes", "srl_boxes_lens"):
                keep.append(items[k].contiguous())
            a.gt_in, a.num_box, a.target_cmp, a.srl_boxes_in, a.srl_boxes_lens = (L.ptr(t) for t in keep[-5:])
            a.gt_out = L.ptr(dst("pad_gt_bboxs", (B, G, 5), torch.float32))
            a.num_box_out = L.ptr(dst("num_box", (B,), torch.int64))
            a.srl_boxes_out = L.ptr(dst("srl_boxes", tuple(sb.shape), torch.int64))
            a.frm_out = L.ptr(dst("pad_frm_mask", (B, ncmp * NPv, G), torch.uint8))
            a.G, a.nv, a.nsrl, a.nbox = G, sb.shape[1], sb.shape[2], sb.shape[3]
        a.B, a.ncmp, a.nfrm0, a.nppf0 = B, ncmp, self.nfrm0, self.nppf0
        a.prop_dim, a.seg_dim = R.shape[-1], S.shape[-1]
        a.conc_type, a.vid_w = L.CONC_TYPE[self.conc_type], self.vid_w
        out["_keepalive"] = keep
        return a, out


BANK_KEYS = ("pad_proposals", "pad_region_feature", "seg_feature_for_frms", "pad_pnt_mask", "pad_gt_bboxs", "num_box")
PER_QUERY_KEYS = ("target_cmp", "srl_boxes", "srl_boxes_lens")


class FeatureBank:
    """The per-video items of a whole dataset in device memory; a batch is `index` [B, ncmp] (rows of the bank) plus the
    per-query keys, and `vog_assemble_from_bank` (csrc/assemble.hip) gathers and assembles it in front of the forward - what
    `DeviceBatchAssembler` does with items that travel over the host link every time (a video segment is the target of its own
    queries, a contrastive sample of others, and every epoch repeats all of them: 2.1 MB per cfg-2 query, again and again).

    Tables of `n_videos` rows, allocated once (addresses never change: fed graphs capture them): region features
    [V, NPv, prop_dim] and segment features [V, nfrm0, seg_dim] in `dtype` ("f32", or "f16": half the footprint, rounded on the
    device by the encoders' own cast, see `lossless_for`), proposals [V, NPv, 7] fp32, padding mask [V, NPv] u8, gt boxes
    [V, G, 5] fp32, box counts [V] i64. `conc_type` sep / svsq: the plain gather to [B, ncmp, ...], plus each video's own frame
    mask `pad_frm_mask` [B, ncmp, NPv, G] with the loss keys (real proposals = up to the last nonzero byte of `pad_pnt_mask`).
    (reference: `AV_CS.itemcollector` + `verb_item_getter_*`, code/dat_loader_simple.py:1046-1510, behind `simple_item_getter`)"""

    # the names under which an assembled batch carries the two feature arrays (`EncodedBank`: the encoder outputs' names)
    region_key, seg_key = "pad_region_feature", "seg_feature_for_frms"

    @property
    def fwd_keys(self):
        """The forward's inputs this bank's assembly writes (`FWD_KEYS` under this bank's names)."""
        return ("pad_proposals", self.region_key, self.seg_key)

    def __init__(self, cfg, comm, n_videos: int, dtype: str = "f32", device=None, prop_dim: Optional[int] = None,
                 seg_dim: Optional[int] = None, n_gt: Optional[int] = None):
        if dtype not in L.BANK_DTYPE:
            raise ValueError(f"FeatureBank dtype must be 'f32' or 'f16', not {dtype!r} (bf16 storage is not lossless under the f16 encoders)")
        self.conc_type = cfg.ds.conc_type
        self.nfrm0 = int(cfg.ds.num_sampled_frm)
        self.nppf0 = int(comm["num_prop_per_frm"])
        self.vid_w = float(cfg.ds.resized_width)
        self.prop_dim = int(prop_dim if prop_dim is not None else cfg.mdl.prop_feat_dim)
        self.seg_dim = int(seg_dim if seg_dim is not None else cfg.mdl.seg_feat_dim)
        self.G = int(n_gt if n_gt is not None else cfg.ds.max_gt_box)
        self.V, self.dtype = int(n_videos), dtype
        q = 8 if dtype == "f16" else 4
        if self.V <= 0 or self.V >= 2 ** 31:
            raise ValueError(f"FeatureBank: n_videos = {n_videos}")
        if self.prop_dim % q or self.seg_dim % q:
            raise ValueError(f"FeatureBank({dtype}): prop_dim / seg_dim must be multiples of {q} (16-byte loads), got "
                             f"{self.prop_dim} / {self.seg_dim}")
        self.NPv = self.nfrm0 * self.nppf0
        self.nbytes = self.V * self.bytes_per_video(self.nppf0, self.prop_dim, self.seg_dim, self.G, dtype, nfrm0=self.nfrm0)
        self.lib = L.load()                          # (no library, no bank: there is no host fallback)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        ft = torch.float16 if dtype == "f16" else torch.float32
        V, NPv, dev = self.V, self.NPv, self.device
        self.tab = {"pad_region_feature": torch.zeros(V, NPv, self.prop_dim, dtype=ft, device=dev),
                    "seg_feature_for_frms": torch.zeros(V, self.nfrm0, self.seg_dim, dtype=ft, device=dev),
                    "pad_proposals": torch.zeros(V, NPv, 7, dtype=torch.float32, device=dev),
                    "pad_pnt_mask": torch.zeros(V, NPv, dtype=torch.uint8, device=dev),
                    "pad_gt_bboxs": torch.zeros(V, self.G, 5, dtype=torch.float32, device=dev),
                    "num_box": torch.zeros(V, dtype=torch.int64, device=dev)}
        self._bad = torch.zeros(16, dtype=torch.int32).pin_memory()          # sticky: a launch saw an index outside [0, V)

    @staticmethod
    def bytes_per_video(nppf0: int, prop_dim: int, seg_dim: int, G: int, dtype: str = "f32", nfrm0: int = 10) -> int:
        """Bytes one video segment occupies: the feature block (`feature_elements` of `dtype`: 532,480 B fp32 / 266,240 B
        f16 at gt5, 8,314,880 / 4,157,440 B at p100) plus the small tables (proposals, padding mask, G gt boxes, box count:
        3.5 KB at gt5, 31 KB at p100)."""
        if dtype not in L.BANK_DTYPE:
            raise ValueError(f"dtype must be 'f32' or 'f16', not {dtype!r}")
        NPv = nfrm0 * nppf0
        return FeatureBank.feature_elements(nppf0, prop_dim, seg_dim, nfrm0) * (2 if dtype == "f16" else 4) + NPv * 7 * 4 + NPv + G * 5 * 4 + 8

    @staticmethod
    def feature_elements(nppf0: int, prop_dim: int, seg_dim: int, nfrm0: int = 10) -> int:
        return nfrm0 * (nppf0 * prop_dim + seg_dim)

    def put(self, start: int, items: Dict[str, torch.Tensor]) -> "FeatureBank":
        """Per-video items [n, ...] (host or device; features fp32) -> rows start .. start + n. f16 banks round on the device
        with the encoders' own cast (vog_cast_f32_to_t16, one RNE rounding)."""
        ts = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in items.items() if k in self.tab}
        for k in ("pad_proposals", "pad_region_feature", "seg_feature_for_frms"):
            if k not in ts:
                raise ValueError(f"FeatureBank.put: items lack '{k}'")
        n = ts["pad_proposals"].shape[0]
        if start < 0 or start + n > self.V:
            raise ValueError(f"FeatureBank.put: rows {start} .. {start + n} of a bank of {self.V}")
        for k, v in ts.items():
            want = (n,) + tuple(self.tab[k].shape[1:])
            if tuple(v.shape) != want:
                raise ValueError(f"FeatureBank.put: '{k}' has shape {tuple(v.shape)}, expected {want}")
            if k in ("pad_region_feature", "seg_feature_for_frms") and v.dtype != torch.float32:
                raise ValueError(f"FeatureBank.put: '{k}' must be float32")
        with torch.cuda.device(self.device):
            for k, v in ts.items():
                dst = self.tab[k][start:start + n]
                if k in ("pad_region_feature", "seg_feature_for_frms"):
                    if self.dtype == "f16":
                        src = v.to(self.device, non_blocking=True).contiguous()
                        L.check(self.lib.vog_cast_f32_to_t16(src.data_ptr(), dst.data_ptr(), src.numel(), None, None, 0,
                                                             L.VOG_F16, L.stream_ptr()), "vog_cast_f32_to_t16")
                        continue
                dst.copy_(v.to(dst.dtype) if v.dtype != dst.dtype else v, non_blocking=True)
        return self

    def lossless_for(self, engine) -> bool:
        """Does a forward from this bank equal the forward from the fp32 features bit for bit? Always for an f32 bank; for an
        f16 bank under the 16-bit plans, whose encoders round every feature to f16 before any use (engine.py:
        d.enc_dtype = VOG_F16 for tx_dtype f16 and bf16). Under "split" / "f32" the result equals the same path on the
        f16-rounded features."""
        return self.dtype == "f32" or engine.plan in ("f16", "bf16")

    def check(self) -> None:
        """Raise VogError if a launch since the last check saw an index outside [0, V) (its rows were written as zeros). Host
        read of pinned memory: call it after synchronising to judge the launches before that point."""
        if int(self._bad[0]) != 0:
            self._bad[0] = 0
            raise L.VogError(f"FeatureBank: a batch named a video outside [0, {self.V}); its rows were zero-filled")

    def _index(self, index):
        """index [B, ncmp] -> an int32 tensor the kernels can read (device, or pinned host: zero copy); host values are
        range-checked here."""
        t = index if isinstance(index, torch.Tensor) else torch.as_tensor(index)
        if t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"FeatureBank: index must be [B, ncmp] int32 / int64, got {tuple(t.shape)} {t.dtype}")
        if not t.is_cuda:
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.V):
                raise ValueError(f"FeatureBank: index outside [0, {self.V})")
            if not (t.is_pinned() and t.dtype == torch.int32 and t.is_contiguous()):
                t = t.to(torch.int32).to(self.device, non_blocking=False)
        return t.to(torch.int32).contiguous() if t.is_cuda else t

    def __call__(self, index, per_query: Optional[Dict[str, torch.Tensor]] = None, out: Optional[Dict[str, torch.Tensor]] = None,
                 with_loss_keys: bool = True, sep_frm_mask: bool = False) -> Dict[str, torch.Tensor]:
        a, out = self.args(index, per_query, out, with_loss_keys, sep_frm_mask)
        with torch.cuda.device(self.device):
            L.check(self.lib.vog_assemble_from_bank(C.byref(a), L.stream_ptr()), "vog_assemble_from_bank")
        return out

    def args(self, index, per_query: Optional[Dict[str, torch.Tensor]] = None, out: Optional[Dict[str, torch.Tensor]] = None,
             with_loss_keys: bool = True, sep_frm_mask: bool = False):
        """The vog_bank_assemble_args of this call and the destination dict, without launching (`engine.Slot.feed_from`
        captures the launch into its graph). `per_query`: target_cmp [B], srl_boxes / srl_boxes_lens [B, nv, nsrl, nbox]
        (device or pinned host) - needed for the loss keys of spat / temp. `out`: optional existing destination tensors.
        `sep_frm_mask` (sep / svsq, with the loss keys): also write `pad_frm_mask` [B, ncmp, NPv, G], the per-video frame
        masks `LossB_SEP` reads (`loader()` batches carry it; the plain gather stays the default). The bank keeps no
        proposal count: a video's real proposals end behind the last NONZERO byte of its `pad_pnt_mask` row. A video whose
        last real proposals are excluded ones (pnt = 0) therefore gets 1 in their rows where the reference loader writes
        the frame comparison - bytes the loss never sees, since it multiplies them by that zero `pad_pnt_mask`, but not
        the reference's bytes."""
        idx = self._index(index)
        B, ncmp = idx.shape
        sep = self.conc_type in ("sep", "svsq")
        NPv, dev = self.NPv, self.device
        out = dict(out or {})
        keep = [idx]
        if with_loss_keys and not sep:
            missing = [k for k in PER_QUERY_KEYS if k not in (per_query or {})]
            if missing:
                raise ValueError(f"FeatureBank: the loss keys of a {self.conc_type} batch need per_query{missing}")

        def dst(k, shape, dtype):
            t = out.get(k)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
                out[k] = t
            assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_cuda and t.is_contiguous(), k
            return t

        lead = (lambda n: (B, ncmp, n)) if sep else (lambda n: (B, ncmp * n))
        a = L.BankAssembleArgs()
        bk = a.bank
        bk.region, bk.seg, bk.props = (L.ptr(self.tab[k]) for k in ("pad_region_feature", "seg_feature_for_frms", "pad_proposals"))
        bk.pnt, bk.gt, bk.num_box = (L.ptr(self.tab[k]) for k in ("pad_pnt_mask", "pad_gt_bboxs", "num_box"))
        bk.V, bk.feat_dtype = self.V, L.BANK_DTYPE[self.dtype]
        a.index = L.ptr(idx)
        a.props_out = L.ptr(dst("pad_proposals", lead(NPv) + (7,), torch.float32))
        a.region_out = L.ptr(dst(self.region_key, lead(NPv) + (self.prop_dim,), torch.float32))
        a.seg_out = L.ptr(dst(self.seg_key, lead(self.nfrm0) + (self.seg_dim,), torch.float32))
        if with_loss_keys or "pad_pnt_mask" in out:
            a.pnt_out = L.ptr(dst("pad_pnt_mask", lead(NPv), torch.uint8))
        if with_loss_keys and sep:
            a.gt_out = L.ptr(dst("pad_gt_bboxs", (B, ncmp, self.G, 5), torch.float32))
            a.num_box_out = L.ptr(dst("num_box", (B, ncmp), torch.int64))
            if sep_frm_mask:
                a.frm_out = L.ptr(dst("pad_frm_mask", (B, ncmp, NPv, self.G), torch.uint8))     # per video, as the loader pads it
        elif with_loss_keys:
            pq = per_query
            for k in PER_QUERY_KEYS:
                t = pq[k] if isinstance(pq[k], torch.Tensor) else torch.from_numpy(pq[k])
                if not (t.is_cuda or t.is_pinned()):
                    t = t.to(dev)
                if t.dtype != torch.int64:
                    raise ValueError(f"FeatureBank: per_query['{k}'] must be int64")
                keep.append(t.contiguous())
            tc, sb, sl = keep[-3:]
            if tuple(tc.shape) != (B,) or sb.dim() != 4 or sb.shape[0] != B or sl.shape != sb.shape:
                raise ValueError("FeatureBank: per_query shapes do not match index")
            a.target_cmp, a.srl_boxes_in, a.srl_boxes_lens = L.ptr(tc), L.ptr(sb), L.ptr(sl)
            a.gt_out = L.ptr(dst("pad_gt_bboxs", (B, self.G, 5), torch.float32))
            a.num_box_out = L.ptr(dst("num_box", (B,), torch.int64))
            a.srl_boxes_out = L.ptr(dst("srl_boxes", tuple(sb.shape), torch.int64))
            a.frm_out = L.ptr(dst("pad_frm_mask", (B, ncmp * NPv, self.G), torch.uint8))
            a.nv, a.nsrl, a.nbox = sb.shape[1], sb.shape[2], sb.shape[3]
        a.bad_index = self._bad.data_ptr()
        a.G = self.G
        a.B, a.ncmp, a.nfrm0, a.nppf0 = B, ncmp, self.nfrm0, self.nppf0
        a.prop_dim, a.seg_dim = self.prop_dim, self.seg_dim
        a.conc_type, a.vid_w = L.CONC_TYPE[self.conc_type], self.vid_w
        out["_keepalive"] = keep
        return a, out

    def loader(self, index_loader) -> "BankLoader":
        """Index batches (dicts with `vid_index` [B, ncmp], the per-query keys and whatever else the model, the loss and the
        evaluator read: language arrays, masks, ids) -> device batches, freshly allocated per batch on the current stream.
        `DevicePrefetcher` passes device batches through untouched, so `Evaluator.forward` and `Learner.train_epoch` run on
        it as on any loader; it can be iterated once per epoch."""
        return BankLoader(self, index_loader)


class CheckpointBound:
    """Mixin (in front of `FeatureBank` / `QueryBank`) of the banks whose rows the engine's own kernels computed: the rows belong
    to one engine, checkpoint (`weights_epoch`), operand plan and geometry, recorded here. `stale` says when any of them has
    moved, `check()` then raises, `refresh` re-encodes from `source`, the bank the rows were derived from (if kept). A subclass
    supplies `SOURCE` (what messages call that bank), `_bind(engine, *geometry)` (validate, then `_bound`), `_check_source(src)`
    and `_reencode(src)`."""
    engine, epoch, plan, geometry, source, encode_seconds = None, -1, None, None, None, 0.0

    def _bound(self, engine, geometry) -> None:
        self.engine, self.geometry = engine, tuple(int(x) for x in geometry)
        self.epoch, self.plan = engine.weights_epoch, engine.plan

    def stale(self, engine=None) -> bool:
        e = engine if engine is not None else self.engine
        return e is None or e is not self.engine or e.weights_epoch != self.epoch or e.plan != self.plan

    def lossless_for(self, engine) -> bool:
        """The rows are the bits `engine`'s kernels compute, while its weights and plan are the ones they were made with."""
        return not self.stale(engine)

    def check(self) -> None:
        """The parent's bad-index report, and: raise VogError when the engine's weights or plan moved since the rows were encoded
        (every batch made from them since then carries another checkpoint's rows)."""
        super().check()
        if self.stale():
            raise L.VogError(f"{type(self).__name__}: the engine's weights or precision plan changed since these rows were encoded "
                             f"(epoch {self.epoch} / plan {self.plan} -> {getattr(self.engine, 'weights_epoch', None)} / "
                             f"{getattr(self.engine, 'plan', None)}): call refresh()")

    def refresh(self, source=None, engine=None):
        """Re-encode every row from `source` (default: the bank `encode` kept) on `engine`'s current weights and plan."""
        src = source if source is not None else self.source
        if src is None:
            raise L.VogError(f"{type(self).__name__}.refresh needs {self.SOURCE} (this one kept none): rebuild it with encode")
        self._check_source(src)
        import time
        self._bind(engine if engine is not None else self.engine, *self.geometry)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self._reencode(src)
            torch.cuda.synchronize()
            self.encode_seconds = time.perf_counter() - t0
        return self


class EncodedBank(CheckpointBound, FeatureBank):
    """A `FeatureBank` of ENCODER OUTPUTS: per video relu(prop_encoder(region rows)) [NPv, prop_enc] and
    relu(seg_encoder(segment rows)) [nfrm0, seg_enc], fp32, computed once per checkpoint by the engine's own encoder kernels
    (`VogEngine.encode_videos` -> vog_ctx_encode_videos) - for runs that keep the weights fixed (validation, test, serving),
    where the raw path re-encodes a video for every query and contrastive slot that names it. 1.03 MB per 100-proposal video
    against 4.16 MB of f16 features; 51 KB against 266 KB at gt5. Everything else is the parent's: the same tables, the same
    vog_assemble_from_bank gather (rows of prop_enc / seg_enc fp32 elements), every conc type, the loss keys, `loader`, `args`,
    bad-index handling. Its assembled feature keys are `enc_region_feature` / `enc_seg_feature` (engine.ENC_KEYS), which the
    forward reads in place of the raw ones: outputs equal the raw path's bit for bit at the geometry (B, ncmp) the rows were
    encoded for (the encoders are row-local, and the kernels that ran are the ones a forward of that geometry runs).
    fp32 rows: the transformers' residual stream starts from the fp32 encoder output, so 16-bit rows would be lossy.
    The rows belong to one checkpoint and one operand plan: the bank records the engine's `weights_epoch` and `plan`, `check()`
    raises when either has moved and `refresh` re-encodes. Training reads the raw features while an encoder is
    being trained; `FP32Trainer` takes these rows once the `enc` stage is frozen."""
    region_key, seg_key = ENC_KEYS
    SOURCE = "the raw bank"

    def __init__(self, cfg, comm, n_videos: int, device=None, n_gt: Optional[int] = None, row_dim: Optional[int] = None):
        """`row_dim`: the width of a proposal row where it is not prop_encode_size (`ObjBank`)."""
        super().__init__(cfg, comm, n_videos, dtype="f32", device=device,
                         prop_dim=int(row_dim if row_dim is not None else cfg.mdl.vsrl.prop_encode_size),
                         seg_dim=int(cfg.mdl.vsrl.seg_encode_size), n_gt=n_gt)

    @staticmethod
    def bytes_per_video(nppf0: int, prop_enc: int, seg_enc: int, G: int, dtype: str = "f32", nfrm0: int = 10) -> int:
        """Bytes one video segment occupies: nfrm0 * (nppf0 * prop_enc + seg_enc) fp32 encodings (51,200 + 10,240 B at gt5,
        1,024,000 + 10,240 B at p100, encode sizes 256) plus the parent's small tables."""
        if dtype != "f32":
            raise ValueError("EncodedBank rows are fp32 (16-bit rows would be lossy: the fp32 residual stream starts from them)")
        return FeatureBank.bytes_per_video(nppf0, prop_enc, seg_enc, G, "f32", nfrm0=nfrm0)

    @staticmethod
    def _row_dim(d) -> int:
        return int(d.prop_enc)

    def _bind(self, engine, B: int, ncmp: int) -> None:
        d, name = engine.desc, type(self).__name__
        if (self._row_dim(d), int(d.seg_enc), int(d.nfrm0), int(d.nppf0)) != (self.prop_dim, self.seg_dim, self.nfrm0, self.nppf0):
            raise ValueError(f"{name}: the engine's model does not have this bank's encode sizes / frame geometry")
        if int(B) <= 0 or int(ncmp) <= 0:
            raise ValueError(f"{name}: geometry B = {B}, ncmp = {ncmp}")
        self._bound(engine, (B, ncmp))

    def _encode_chunk(self, region, seg, props, B: int, ncmp: int):
        """One pseudo-batch of raw rows -> (proposal rows, segment rows) of this bank."""
        return self.engine.encode_videos(region, seg, B, ncmp)

    def _encode_rows(self, start: int, region: torch.Tensor, seg: torch.Tensor) -> None:
        """Raw rows of n videos (device; f16 bank rows widen exactly) -> encoded rows start .. start + n, in chunks of
        B * ncmp videos - one pseudo-batch of the bound geometry each; a short last chunk is filled up with its first video.
        The boxes that go with them are this bank's own `pad_proposals` rows start .. start + n (written before the features, by
        `encode` and `from_items` alike)."""
        B, ncmp = self.geometry
        per = B * ncmp
        n = int(region.shape[0])
        props = self.tab["pad_proposals"][start:start + n]
        for s0 in range(0, n, per):
            rows = [t[s0:s0 + per].float() for t in (region, seg, props)]
            m = int(rows[0].shape[0])
            if m < per:
                rows = [torch.cat([t, t[:1].expand(per - m, -1, -1)]) for t in rows]
            er, es = self._encode_chunk(*rows, B, ncmp)
            self.tab["pad_region_feature"][start + s0:start + s0 + m].copy_(er[:m])      # (the tables keep the parent's names)
            self.tab["seg_feature_for_frms"][start + s0:start + s0 + m].copy_(es[:m])

    def put(self, start: int, items):
        raise TypeError("EncodedBank rows are written by encode / from_items / refresh (raw features go through the engine's encoders)")

    @classmethod
    def encode(cls, raw_bank: FeatureBank, engine, B: int, ncmp: int, keep_source: bool = True) -> "EncodedBank":
        """The encoded counterpart of `raw_bank` for forwards of geometry (B, ncmp) on `engine`'s current weights: the small
        tables are copied, the feature rows go chunk by chunk through vog_ctx_encode_videos. `keep_source`: remember the raw
        bank so that `refresh()` (and `Learner.validate`) can re-encode after the weights moved."""
        if isinstance(raw_bank, EncodedBank):
            raise ValueError("EncodedBank.encode takes a bank of raw features")
        self = cls(engine.cfg, {"num_prop_per_frm": raw_bank.nppf0}, raw_bank.V, device=raw_bank.device, n_gt=raw_bank.G)
        if (self.conc_type, self.nfrm0) != (raw_bank.conc_type, raw_bank.nfrm0):
            raise ValueError("EncodedBank.encode: the engine's configuration does not match the raw bank's")
        for k in ("pad_proposals", "pad_pnt_mask", "pad_gt_bboxs", "num_box"):
            self.tab[k].copy_(raw_bank.tab[k])
        self.source = raw_bank if keep_source else None
        self._bind(engine, B, ncmp)
        self.refresh(raw_bank, engine)
        return self

    @classmethod
    def from_items(cls, cfg, comm, n_videos: int, chunks, engine, B: int, ncmp: int, device=None, n_gt: Optional[int] = None):
        """The same from host items, so that the raw features never live on the device as a bank: `chunks` yields
        (start, items) with per-video items [n, ...] as `FeatureBank.put` takes them (features fp32)."""
        self = cls(cfg, comm, n_videos, device=device, n_gt=n_gt)
        self._bind(engine, B, ncmp)
        for start, items in chunks:
            ts = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in items.items() if k in self.tab}
            feats = {k: ts.pop(k) for k in ("pad_region_feature", "seg_feature_for_frms") if k in ts}
            n = int(ts["pad_proposals"].shape[0]) if "pad_proposals" in ts else -1
            want = {"pad_region_feature": (n, self.NPv), "seg_feature_for_frms": (n, self.nfrm0)}
            for k, w in want.items():
                if k not in feats or feats[k].dtype != torch.float32 or tuple(feats[k].shape[:2]) != w:
                    raise ValueError(f"EncodedBank.from_items: '{k}' must be float32 {w + ('dim',)}")
            if start < 0 or start + n > self.V:
                raise ValueError(f"EncodedBank.from_items: rows {start} .. {start + n} of a bank of {self.V}")
            with torch.cuda.device(self.device):
                for k, v in ts.items():
                    self.tab[k][start:start + n].copy_(v.to(self.tab[k].dtype), non_blocking=True)
                self._encode_rows(start, feats["pad_region_feature"].to(self.device), feats["seg_feature_for_frms"].to(self.device))
        return self

    def _check_source(self, raw: FeatureBank) -> None:
        if raw.V != self.V or raw.NPv != self.NPv:
            raise ValueError(f"{type(self).__name__}.refresh: the raw bank does not have this bank's videos")

    def _reencode(self, raw: FeatureBank) -> None:
        self._encode_rows(0, raw.tab["pad_region_feature"], raw.tab["seg_feature_for_frms"])


class ObjBank(EncodedBank):
    """An `EncodedBank` one stage further down, for sep / svsq models with an object transformer: per video the OUTPUT ROWS OF
    obj_tx's last layer [NPv, prop_enc + seg_enc] and relu(seg_encoder(segment rows)) [nfrm0, seg_enc] (the sep head reads the
    segment encodings), fp32, computed once per checkpoint by the engine's own kernels (`VogEngine.obj_videos` ->
    vog_ctx_obj_videos). There every video is its own sequence set, obj_tx has no mask and no per-slot box offset, so its
    output depends on the video and the checkpoint alone - and the raw and the encoded path recompute it for every query and
    contrastive slot that names the video. 112,640 B of rows per gt5 video (encoded bank: 61,440 B), 2,058,240 B at 100
    proposals per frame. Everything else is the parent's: the tables, the vog_assemble_from_bank gather, the binding to one
    engine, checkpoint, plan and geometry (B, ncmp), `encode` / `from_items` / `stale` / `check` / `refresh`, `loader`,
    bad-index handling. Its assembled feature keys are `obj_region_feature` / `enc_seg_feature` (engine.OBJ_KEYS); a forward
    from them starts at mul_tx. It equals the raw path's bit for bit while a batch has no more rows than one band of the fused
    encoder-layer tail (`VogEngine.obj_band_rows`: 512 rows = 10 gt5 videos, 256 on the hi + lo plan; any size where the tail
    runs as separate launches) - `lossless_for` says which. Beyond that the tail's fp32 summation order depends on the band a
    video's rows lie in, a bank row carries the order of the slot it was encoded at, and outputs agree with the raw path's to
    the last bits of those sums (measured: 1e-4 on the rows), not bit for bit. Forwards served from the bank never run obj_tx, so
    `encode` / `refresh` report its logits themselves: obj_videos folds them into the engine's statistics, and after its
    synchronisation `refresh` asks `check_logit_scale()` - if that raised the plan, the rows are encoded once more under the
    new one before the bank counts as fresh. Not for spat / temp (obj_tx attends across the videos of a query), for
    training only with the `enc` and `obj` stages frozen (`FP32Trainer(freeze=)`)."""
    region_key, seg_key = OBJ_KEYS

    def __init__(self, cfg, comm, n_videos: int, device=None, n_gt: Optional[int] = None):
        has_obj = cfg.mdl.name == "vgrnd" or (cfg.mdl.name == "vog" and bool(cfg.mdl.obj_tx.to_use))
        if cfg.ds.conc_type not in ("sep", "svsq") or not has_obj:
            raise ValueError(f"ObjBank ({cfg.mdl.name}, {cfg.ds.conc_type}): {OBJ_MODEL_RULE}")
        super().__init__(cfg, comm, n_videos, device=device, n_gt=n_gt,
                         row_dim=int(cfg.mdl.vsrl.prop_encode_size) + int(cfg.mdl.vsrl.seg_encode_size))
        # (the parent sized itself through this class's bytes_per_video, whose arguments are the two encode sizes)
        self.nbytes = self.V * FeatureBank.bytes_per_video(self.nppf0, self.prop_dim, self.seg_dim, self.G, "f32", nfrm0=self.nfrm0)

    @staticmethod
    def bytes_per_video(nppf0: int, prop_enc: int, seg_enc: int, G: int, dtype: str = "f32", nfrm0: int = 10) -> int:
        """Bytes one video segment occupies: nfrm0 * (nppf0 * (prop_enc + seg_enc) + seg_enc) fp32 values (102,400 + 10,240 B at
        gt5, 2,048,000 + 10,240 B at p100, encode sizes 256) plus the parent's small tables."""
        if dtype != "f32":
            raise ValueError("ObjBank rows are fp32 (16-bit rows would be lossy: mul_tx's fp32 residual stream starts from them)")
        return FeatureBank.bytes_per_video(nppf0, prop_enc + seg_enc, seg_enc, G, "f32", nfrm0=nfrm0)

    @staticmethod
    def _row_dim(d) -> int:
        return int(d.prop_enc) + int(d.seg_enc)

    def _bind(self, engine, B: int, ncmp: int) -> None:
        if not (engine.sep and engine.has_obj_tx):
            raise ValueError(f"ObjBank: {OBJ_MODEL_RULE}")
        super()._bind(engine, B, ncmp)

    def _encode_chunk(self, region, seg, props, B: int, ncmp: int):
        """Through encoders AND obj_tx, whose relative-position bias reads the boxes."""
        return self.engine.obj_videos(region, seg, props, B, ncmp)

    def lossless_for(self, engine) -> bool:
        """Bit-equal to the raw path: fresh rows, and a geometry whose rows fit one band of the fused tail (see the class)."""
        if self.stale(engine):
            return False
        band = engine.obj_band_rows()
        return band == 0 or self.geometry[0] * self.geometry[1] * self.NPv <= band

    def refresh(self, source: Optional[FeatureBank] = None, engine=None) -> "ObjBank":
        super().refresh(source, engine)
        # (synchronised by now) the logits obj_tx saw while the rows were made, against the plan they were made under
        self.engine.check_logit_scale()
        if self.stale():                        # the plan rose: once more, under the new one
            super().refresh(source, self.engine)
        return self


def _assemble_into(dev: Dict[str, torch.Tensor], bank: FeatureBank, index) -> None:
    """The bank half of a loader's step: the assembly of `index` behind the per-query keys `dev` already holds."""
    res = bank(index, dev, with_loss_keys=True, sep_frm_mask=True)
    res.pop("_keepalive", None)
    dev.update(res)


class BankLoader:
    def __init__(self, bank: FeatureBank, index_loader):
        self.bank, self.index_loader = bank, index_loader

    def __len__(self):
        return len(self.index_loader)

    def __iter__(self):
        bank = self.bank
        for bt in self.index_loader:
            t = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in bt.items()}
            index = t.pop("vid_index")
            with torch.cuda.device(bank.device):
                dev = {k: v.to(bank.device, non_blocking=True) for k, v in t.items()}
                _assemble_into(dev, bank, index)
            yield dev
        bank.check()


def _row_spec(v):
    """(row shape, torch dtype) of a spec entry: an example batch [n, ...] (tensor / array) or a (row_shape, dtype) pair."""
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], torch.dtype):
        return tuple(int(x) for x in v[0]), v[1]
    t = v if isinstance(v, torch.Tensor) else torch.from_numpy(v)
    return tuple(t.shape[1:]), t.dtype


class QueryBank:
    """The per-query part of a whole dataset in device memory - language arrays, masks, `target_cmp`, `srl_boxes`,
    `srl_boxes_lens`, the metric columns, optionally `vid_index`: 2.1 to 2.3 KB per query, about 46 MB for 20 000 queries. A
    batch is `qry_index` [B] (rows of the bank) and `vog_gather_rows` (csrc/assemble.hip) writes every key's rows into the
    batch's buffers in ONE launch - what the host otherwise does with one small copy per key and step.

    Tables `[Q, ...]`, one per key of `spec` (name -> example batch [n, ...], or (row shape, dtype)), allocated once: addresses
    never change, fed graphs capture them. `host_keys`: columns that are ALSO kept on the host as numpy arrays (`meta`), by
    default the evaluator's metadata keys, so that its records' metadata never touches the device.
    Override rule (here and in `engine.Slot.feed_from`): a key present in the index batch / staging buffer is used from there,
    a key absent there and present in the bank is gathered."""

    def __init__(self, n_queries: int, spec, device=None, host_keys=None):
        self.Q = int(n_queries)
        if self.Q <= 0 or self.Q >= 2 ** 31:
            raise ValueError(f"QueryBank: n_queries = {n_queries}")
        self.spec = {k: _row_spec(v) for k, v in spec.items()}
        if not self.spec:
            raise ValueError("QueryBank: no keys")
        if host_keys is None:
            from .eval_vsrl_corr import Evaluator
            host_keys = [k for k in Evaluator.META_KEYS if k in self.spec]
        self.host_keys = tuple(host_keys)
        for k in self.host_keys:
            if k not in self.spec:
                raise ValueError(f"QueryBank: host key '{k}' is not in the spec")
        self.lib = L.load()                          # (no library, no bank: there is no host fallback)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.tab = {k: torch.zeros((self.Q,) + shp, dtype=dt, device=self.device) for k, (shp, dt) in self.spec.items()}
        self.host = {k: torch.zeros((self.Q,) + self.spec[k][0], dtype=self.spec[k][1]).numpy() for k in self.host_keys}
        self._bad = torch.zeros(16, dtype=torch.int32).pin_memory()          # sticky: a launch saw a row outside [0, Q)

    @property
    def keys(self):
        return tuple(self.tab)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tab.values())

    def row_bytes(self, k: str) -> int:
        t = self.tab[k]
        return (t.numel() // self.Q) * t.element_size()

    @classmethod
    def from_batches(cls, batches, keys=None, host_keys=None, device=None) -> "QueryBank":
        """The rows of a list of host batches, concatenated along axis 0 (the ragged last batch is fewer rows). `keys`: the
        columns to keep (default: every key of the first batch). A key whose row shape or dtype differs between batches is
        refused."""
        bts = [{k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in bt.items()} for bt in batches]
        if not bts:
            raise ValueError("QueryBank.from_batches: no batches")
        keys = list(keys) if keys is not None else list(bts[0])
        spec = {}
        for k in keys:
            for i, bt in enumerate(bts):
                if k not in bt:
                    raise ValueError(f"QueryBank.from_batches: batch {i} lacks '{k}'")
                rs = (tuple(bt[k].shape[1:]), bt[k].dtype)
                if spec.setdefault(k, rs) != rs:
                    raise ValueError(f"QueryBank.from_batches: '{k}' has rows of {rs[0]} {rs[1]} in batch {i}, "
                                     f"{spec[k][0]} {spec[k][1]} before")
        sizes = [int(bt[keys[0]].shape[0]) for bt in bts]
        for k in keys:
            if [int(bt[k].shape[0]) for bt in bts] != sizes:
                raise ValueError(f"QueryBank.from_batches: '{k}' does not have the batch sizes of '{keys[0]}'")
        if host_keys is None:
            from .eval_vsrl_corr import Evaluator
            host_keys = [k for k in Evaluator.META_KEYS if k in spec]
        qb = cls(sum(sizes), spec, device=device, host_keys=host_keys)
        qb.put(0, {k: torch.cat([bt[k] for bt in bts], dim=0) for k in keys})
        return qb

    def put(self, start: int, items) -> "QueryBank":
        """Per-query rows [n, ...] (host or device) -> rows start .. start + n of the tables (and of the host columns)."""
        ts = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in items.items() if k in self.tab}
        if not ts:
            raise ValueError("QueryBank.put: none of the items is a key of the bank")
        n = int(next(iter(ts.values())).shape[0])
        if start < 0 or start + n > self.Q:
            raise ValueError(f"QueryBank.put: rows {start} .. {start + n} of a bank of {self.Q}")
        for k, v in ts.items():
            want = (n,) + self.spec[k][0]
            if tuple(v.shape) != want or v.dtype != self.spec[k][1]:
                raise ValueError(f"QueryBank.put: '{k}' is {tuple(v.shape)} {v.dtype}, expected {want} {self.spec[k][1]}")
        for k, v in ts.items():
            if k in self.host:
                self.host[k][start:start + n] = v.detach().cpu().numpy()
            self.tab[k][start:start + n].copy_(v, non_blocking=False)
        return self

    def meta(self, qry_index) -> Dict[str, "object"]:
        """The host columns' rows of `qry_index` (numpy, by fancy indexing): the evaluator's metadata without the device."""
        import numpy as np
        idx = np.asarray(qry_index.cpu() if isinstance(qry_index, torch.Tensor) else qry_index).astype(np.int64).reshape(-1)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.Q):
            raise ValueError(f"QueryBank: index outside [0, {self.Q})")
        return {k: v[idx] for k, v in self.host.items()}

    def check(self) -> None:
        """Raise VogError if a launch since the last check saw a row outside [0, Q) (its rows were written as zeros). Host
        read of pinned memory: call it after synchronising to judge the launches before that point."""
        if int(self._bad[0]) != 0:
            self._bad[0] = 0
            raise L.VogError(f"QueryBank: a batch named a query outside [0, {self.Q}); its rows were zero-filled")

    def _index(self, index):
        """qry_index [B] -> an int32 tensor the kernel can read (device, or pinned host: zero copy); host values are
        range-checked here (as FeatureBank._index)."""
        t = index if isinstance(index, torch.Tensor) else torch.as_tensor(index)
        if t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"QueryBank: qry_index must be [B] int32 / int64, got {tuple(t.shape)} {t.dtype}")
        if not t.is_cuda:
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.Q):
                raise ValueError(f"QueryBank: index outside [0, {self.Q})")
            if not (t.is_pinned() and t.dtype == torch.int32 and t.is_contiguous()):
                t = t.to(torch.int32).to(self.device, non_blocking=False)
        return t.to(torch.int32).contiguous() if t.is_cuda else t

    def args(self, qry_index, out: Optional[Dict[str, torch.Tensor]] = None, staged=(), keys=None):
        """The vog_gather_args of this call and the destination dict, without launching (`engine.Slot.feed_from` captures the
        launch into its graph). `out`: optional existing destination tensors [B, ...] (matched by byte size); missing ones
        are allocated. `keys`: the columns to gather (default: all). `staged`: (src, dst, bytes) address triples that ride
        in the same launch as per-batch keys (plain ranges: keys the caller still stages, the validation step number)."""
        idx = self._index(qry_index)
        B = int(idx.shape[0])
        keys = list(self.tab) if keys is None else list(keys)
        staged = list(staged)
        if B <= 0 or not keys and not staged:
            raise ValueError("QueryBank: an empty gather")
        if len(keys) + len(staged) > L.MAX_GATHER_KEYS:
            raise ValueError(f"QueryBank: {len(keys)} + {len(staged)} keys in one launch (VOG_MAX_GATHER_KEYS = {L.MAX_GATHER_KEYS})")
        out = dict(out or {})
        a = L.GatherArgs()
        a.index, a.B, a.Q = L.ptr(idx), B, self.Q
        n = 0
        for k in keys:
            if k not in self.tab:
                raise KeyError(f"QueryBank: no column '{k}'")
            shp, dt = self.spec[k]
            t = out.get(k)
            if t is None:
                t = torch.empty((B,) + shp, dtype=dt, device=self.device)
                out[k] = t
            rb = self.row_bytes(k)
            assert t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() == B * rb and t.element_size() == self.tab[k].element_size(), k
            a.keys[n].table, a.keys[n].dst, a.keys[n].row_bytes, a.keys[n].per_batch = L.ptr(self.tab[k]), L.ptr(t), rb, 0
            n += 1
        for src, dst, nb in staged:
            a.keys[n].table, a.keys[n].dst, a.keys[n].row_bytes, a.keys[n].per_batch = int(src), int(dst), int(nb), 1
            n += 1
        a.n_keys = n
        a.bad_index = self._bad.data_ptr()
        out["_keepalive"] = [idx]
        return a, out

    def __call__(self, qry_index, out: Optional[Dict[str, torch.Tensor]] = None, keys=None) -> Dict[str, torch.Tensor]:
        a, out = self.args(qry_index, out, keys=keys)
        with torch.cuda.device(self.device):
            L.check(self.lib.vog_gather_rows(C.byref(a), L.stream_ptr()), "vog_gather_rows")
        return out

    def loader(self, index_loader, bank: Optional[FeatureBank] = None) -> "QueryLoader":
        """Index batches (dicts with `qry_index` [B], optionally `vid_index` [B, ncmp] and any key that overrides a column:
        a training epoch with re-sampled contrastive videos sends `vid_index`, `target_cmp` and the permutation keys) ->
        eager device batches, freshly allocated per batch on the current stream. With `bank` (a `FeatureBank`) its assembly
        runs behind the gather - `vid_index` from the index batch or, absent there, from the column - and the batch equals
        `BankLoader`'s on the full index batch."""
        return QueryLoader(self, index_loader, bank)


class LangBank(CheckpointBound, QueryBank):
    """A `QueryBank` whose four word-level columns are replaced by the RESULTS OF THE LANGUAGE CHAIN: per query the argument
    vectors `lang_arg_vec` [nvl, nsrl, lang_enc] and the projected final hidden state `lang_final_hidden` [nvl, lang_enc]
    (engine.ARG_KEYS; nvl = ncmp for sep / svsq and 1 otherwise, where the second column is not kept: only the sep head reads
    it), fp32, computed once per checkpoint by the engine's own kernels (`VogEngine.encode_queries` -> vog_lang_forward) - for
    runs that keep the weights fixed, where every forward otherwise re-runs prologue, two BiLSTM layers, out-projection and
    argument gather on the same query. 5 KB + 1 KB per query at cfg 2 (5 arguments x 256 floats, spat) in place of about
    1.8 KB of int64 word arrays. Everything else is the parent's: the tables, the one vog_gather_rows launch per batch that
    writes `ARG_KEYS` with the other per-query keys, `loader`, `args`, `__call__`, `meta`, bad-index handling (zero rows plus
    the sticky word). A batch gathered from it is in the engine's vector form: its forward starts behind the BiLSTM.
    The rows belong to one checkpoint, one operand plan and one geometry (B, T): the bank records the engine's
    `weights_epoch` and `plan`, `check()` raises when either has moved and `refresh` re-encodes. Training needs the word-level
    keys while the language side is being trained; `FP32Trainer` takes the vectors once the `lang` stage is frozen."""
    WORD_KEYS, SRC_KEYS = WORD_KEYS, LANG_KEYS
    SOURCE = "the query bank of word-level keys"

    @staticmethod
    def bytes_per_query(nsrl: int, lang_enc: int, nvl: int = 1, sep: bool = False) -> int:
        """Bytes of the two columns of one query: nvl * nsrl * lang_enc fp32 argument vectors (5,120 B at cfg 2: 5 arguments x
        256) and, for sep / svsq (where nvl = ncmp), nvl * lang_enc fp32 of the final hidden projection (1,024 B per video)."""
        return 4 * int(nvl) * int(lang_enc) * (int(nsrl) + (1 if sep else 0))

    @classmethod
    def encode(cls, query_bank: QueryBank, engine, B: int, T: int, keep_source: bool = True) -> "LangBank":
        """The vector-form counterpart of `query_bank` for forwards of geometry (B, T) on `engine`'s current weights: every other
        column (and the host columns) is copied, the word-level columns go chunk by chunk through vog_lang_forward.
        `keep_source`: remember the query bank so that `refresh()` (and `Learner.validate`) can re-encode after the weights
        moved."""
        if isinstance(query_bank, LangBank):
            raise ValueError("LangBank.encode takes a bank of word-level keys")
        for k in cls.SRC_KEYS:
            if k not in query_bank.tab:
                raise ValueError(f"LangBank.encode: the query bank lacks '{k}'")
        d = engine.desc
        nvl = int(query_bank.spec["srl_arg_words_ind"][0][0])
        spec = {k: v for k, v in query_bank.spec.items() if k not in cls.WORD_KEYS}
        spec[ARG_KEYS[0]] = ((nvl, int(d.nsrl), int(d.lang_enc)), torch.float32)
        if engine.sep:
            spec[ARG_KEYS[1]] = ((nvl, int(d.lang_enc)), torch.float32)
        self = cls(query_bank.Q, spec, device=query_bank.device, host_keys=[k for k in query_bank.host_keys if k in spec])
        for k in spec:
            if k not in ARG_KEYS:
                self.tab[k].copy_(query_bank.tab[k])
        for k in self.host_keys:
            self.host[k][...] = query_bank.host[k]
        self.source = query_bank if keep_source else None
        self._bind(engine, B, T)
        self.refresh(query_bank, engine)
        return self

    def _bind(self, engine, B: int, T: int) -> None:
        d = engine.desc
        want = (int(d.nsrl), int(d.lang_enc))
        if tuple(self.spec[ARG_KEYS[0]][0][1:]) != want or (ARG_KEYS[1] in self.spec) != bool(engine.sep):
            raise ValueError("LangBank: the engine's model does not have this bank's argument geometry (nsrl, lang_enc, conc type)")
        if int(B) <= 0 or not (1 <= int(T) <= int(d.seq_len)):
            raise ValueError(f"LangBank: geometry B = {B}, T = {T}")
        self._bound(engine, (B, T))

    def put(self, start: int, items) -> "LangBank":
        if any(k in items for k in ARG_KEYS + self.WORD_KEYS):
            raise TypeError("LangBank's argument vectors are written by encode / refresh (word-level keys go through the engine's "
                            "language chain)")
        return super().put(start, items)

    def _check_source(self, src: QueryBank) -> None:
        if src.Q != self.Q:
            raise ValueError("LangBank.refresh: the query bank does not have this bank's queries")

    def _reencode(self, src: QueryBank) -> None:
        lang, fh = self.engine.encode_queries({k: src.tab[k] for k in self.SRC_KEYS}, *self.geometry)
        self.tab[ARG_KEYS[0]].copy_(lang)
        if ARG_KEYS[1] in self.tab:
            self.tab[ARG_KEYS[1]].copy_(fh)

    def refresh(self, source: Optional[QueryBank] = None, engine=None) -> "LangBank":
        super().refresh(source, engine)
        self.engine.check()                     # (a stalled BiLSTM hand-off while encoding: the rows would be NaN)
        return self

    def lossless_for(self, engine) -> bool:
        """The rows are the bits `engine`'s language chain computes for a pseudo-batch of the bound geometry (B, T) - what a
        group member (`make_group`) of that geometry reads - while its weights and plan are the ones they were made with.
        It does NOT promise bit equality with the STAND-ALONE word-form forward, with raw features or with `EncodedBank` rows,
        at the bound (B, T) or elsewhere. Measured (tests/test_gpu_lang_bank.py prints it): the small test models, whose chain
        has one form, are bit-equal (also with encoded rows); at cfg 2 (full/cfg2_vog_spat_gt5_bs4) the logits differ by 2.1e-4
        and the scores by 4.3e-5 - stand-alone the BiLSTM layers project their input in the kernel's prologue and share their
        launches with the visual chain, the language-only chain takes the group encoder's forms, and the fp32 summation
        orders differ; the group test's bound (1.5e-3 on mdl_outs) holds."""
        return not self.stale(engine)


class QueryLoader:
    def __init__(self, queries: QueryBank, index_loader, bank: Optional[FeatureBank] = None):
        self.queries, self.index_loader, self.bank = queries, index_loader, bank

    def __len__(self):
        return len(self.index_loader)

    def __iter__(self):
        qb, bank = self.queries, self.bank
        for bt in self.index_loader:
            t = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)) for k, v in bt.items()}
            qi = t.pop("qry_index")
            with torch.cuda.device(qb.device):
                over = {k: v.to(qb.device, non_blocking=True) for k, v in t.items()}
                dev = qb(qi, keys=[k for k in qb.keys if k not in over])
                dev.pop("_keepalive", None)
                dev.update(over)
                if bank is not None:
                    _assemble_into(dev, bank, dev.pop("vid_index"))
            yield dev
        if bank is not None:
            bank.check()
        qb.check()
