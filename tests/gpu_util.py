"""Shared helpers of the -m gpu parity tests (product path = libvog_hip via ctypes)."""
import importlib

import numpy as np
import torch

from oracle import cases
from oracle import vog_oracle as vo

pkg = importlib.import_module("vognet-pytorch_amd")
L = importlib.import_module("vognet-pytorch_amd.lib")
engine_mod = importlib.import_module("vognet-pytorch_amd.engine")


def rnd16(x: torch.Tensor, dtype: str) -> torch.Tensor:
    t = torch.bfloat16 if dtype == "bf16" else torch.float16
    return x.to(t)


def t16(dtype: str):
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def comm_for(c):
    return {"vocab_size": c["vocab"], "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1},
            "num_prop_per_frm": c["nppf0"]}


_ENGINES = {}
_DEFAULT_OPTIONS = {"lstm_persistent": 1, "lstm_inject_stall": 0, "fused_tail": 1, "fused_enc": 1, "pair_launches": 1, "pair_mask": 15,
                    "fused_ih": 1, "enc_lean": -1}


_CASES = {}


def _case(name):
    """cases.build(name) once per session (0.3-1 s of seeded numpy per call, on ~600 uses): the arrays are shared and must
    not be written to (no test does); cfg is copied because callers set cfg.hip fields."""
    import copy
    hit = _CASES.pop(name, None)
    if hit is None:
        hit = cases.build(name)
        if len(_CASES) >= 10:                       # (a full-size state dict is 177 MB of host memory)
            _CASES.pop(next(iter(_CASES)))
    _CASES[name] = hit                              # (most recently used last)
    cfg, sd, batch, c = hit
    return copy.deepcopy(cfg), dict(sd), dict(batch), dict(c)


def build_engine(name, tx_dtype=None, cached=False):
    """tx_dtype None: the package default (`auto`: f16 kernels inside their envelope, hi + lo operands / the fp32 path beyond;
    engine.py). cached=True (round 6: the launch-structure variant tests, which only flip context options on the same
    checkpoints): the engine of (case, tx_dtype) is built once per session - registering 44 M weights costs ~1 s, most of such a
    test - and handed out with every option back at its default and fresh device inputs; an engine that has seen a stall or
    whose plan was raised at run time is rebuilt."""
    key = (name, tx_dtype)
    hit = _ENGINES.get(key) if cached else None
    if hit is not None and hit[0].stalls == 0 and hit[0].plan == hit[5]:
        eng, cfg, sd, batch, c, _ = hit
        for k, v in _DEFAULT_OPTIONS.items():
            eng.set_option(k, v)
        eng._fault_seen = int(eng._fault[0])
    else:
        cfg, sd, batch, c = _case(name)
        if tx_dtype is not None:
            cfg.hip.tx_dtype = tx_dtype
        eng = engine_mod.VogEngine(cfg, comm_for(c))
        eng.load_state_dict(sd)
        if cached:
            if len(_ENGINES) >= 48:
                _ENGINES.pop(next(iter(_ENGINES)))
            _ENGINES[key] = (eng, cfg, sd, batch, c, eng.plan)
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    return eng, cfg, sd, batch, c, dev


def oracle_run(cfg, sd, batch, c, keep_stages=False):
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    inp = vo.to_torch(batch)
    with torch.no_grad():
        out = vo.forward(oc, vo.to_torch(sd), inp, keep_stages=keep_stages)
        out.update(vo.pred_head(oc, out, inp))
    return out


def rel_err(a: np.ndarray, ref: np.ndarray, floor=1e-6):
    return np.abs(a - ref) / np.maximum(np.abs(ref), floor)


# ---- banks: what the bank test modules share --------------------------------------------------------------------------------
dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
synth = importlib.import_module("vognet-pytorch_amd.synth")
FEATS = ("pad_region_feature", "seg_feature_for_frms")


def video_pool(nv, cfg, c, seed, n_gt=8):
    """`BANK_KEYS` items of nv synthetic videos at the model's feature sizes."""
    it = synth.make_items(nv, 1, c["nppf0"], prop_dim=int(cfg.mdl.prop_feat_dim), seg_dim=int(cfg.mdl.seg_feat_dim), n_gt=n_gt, seed=seed)
    return {k: np.ascontiguousarray(it[k][:, 0]) for k in dls.BANK_KEYS}


def index_batches(batch, cfg, c, nv, n, seed=100):
    Bq, ncmp = batch["num_cmp_msk"].shape
    out = []
    for i in range(n):
        rng = np.random.default_rng(seed + i)
        pq = synth.make_items(Bq, ncmp, 1, prop_dim=4, seg_dim=4, n_gt=8, seed=60 + i)
        small = {k: v for k, v in batch.items() if k not in dls.FWD_KEYS}
        small.update({k: pq[k] for k in dls.PER_QUERY_KEYS})
        idx = rng.integers(0, nv, size=(Bq, ncmp)).astype(np.int32)
        if ncmp > 1 and i == 1:
            idx[0, 1] = idx[0, 0]
        out.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**small, "vid_index": idx}.items()})
    return out


def trace(eng, inp, T):
    b, _, (B, ncmp, T) = eng.make_batch(inp, T)
    return eng.describe_steps(b, eng.workspace(B, ncmp, T))


def flat(trace):
    return [p for n in trace for p in n.split("+")]


def encoded(eng, dev):
    """The batch with its two feature arrays replaced by their encodings (vog_ctx_encode_videos at the batch's geometry). The
    rows of a batch in (video, frame, proposal) order or in the spat / temp concatenation are rows all the same: the encoders
    are row-local and a segment row serves the nppf0 proposal rows that follow it in either layout."""
    B, ncmp = dev["num_cmp_msk"].shape
    d = eng.desc
    r, s = dev["pad_region_feature"], dev["seg_feature_for_frms"]
    before = (r.clone(), s.clone())
    ep, es = eng.encode_videos(r.reshape(B * ncmp, d.nfrm0 * d.nppf0, d.prop_dim), s.reshape(B * ncmp, d.nfrm0, d.seg_dim), B, ncmp)
    torch.cuda.synchronize()
    assert torch.equal(before[0], r) and torch.equal(before[1], s)              # inputs are never modified
    enc = {k: v for k, v in dev.items() if k not in FEATS}
    enc[engine_mod.ENC_KEYS[0]] = ep.reshape(tuple(r.shape[:-1]) + (d.prop_enc,))
    enc[engine_mod.ENC_KEYS[1]] = es.reshape(tuple(s.shape[:-1]) + (d.seg_enc,))
    return enc


def objed(eng, dev):
    """The batch with its two feature arrays replaced by obj_tx's output rows and the segment encodings (vog_ctx_obj_videos at
    the batch's geometry)."""
    B, ncmp = dev["num_cmp_msk"].shape
    d = eng.desc
    r, s, p = dev["pad_region_feature"], dev["seg_feature_for_frms"], dev["pad_proposals"]
    before = (r.clone(), s.clone(), p.clone())
    NPv = d.nfrm0 * d.nppf0
    oo, es = eng.obj_videos(r.reshape(B * ncmp, NPv, d.prop_dim), s.reshape(B * ncmp, d.nfrm0, d.seg_dim), p.reshape(B * ncmp, NPv, 7), B, ncmp)
    torch.cuda.synchronize()
    assert torch.equal(before[0], r) and torch.equal(before[1], s) and torch.equal(before[2], p)      # inputs are never modified
    obj = {k: v for k, v in dev.items() if k not in FEATS}
    obj[engine_mod.OBJ_KEYS[0]] = oo.reshape(tuple(r.shape[:-1]) + (d.prop_enc + d.seg_enc,))
    obj[engine_mod.OBJ_KEYS[1]] = es.reshape(tuple(s.shape[:-1]) + (d.seg_enc,))
    return obj
