"""-m gpu: the forward with the context option `lstm_wide` (one persistent BiLSTM launch per layer for language chains of
17 .. 32 sentences, vog_bilstm_layer_wide) - which launches the builder issues, and the whole forward against the CPU oracle
(oracle/vog_oracle.py, the way bench.py --full checks parity) within the bounds of tests/test_gpu_forward.py: 1e-3 relative on
pred_scores / mdl_outs_eval, 6e-3 absolute on the logits, 4e-3 absolute on fin_scores* / vidf_outs.

Cases (weights and inputs from vognet-pytorch_amd/synth.py, ragged sentences): the small/vog_spat dimensions at B = 32
(32 sentences, R = 32, layer-0 projection as a GEMM launch: a 50-word vocabulary has no gate table), a sep model at B = 8,
ncmp = 4 (32 sentences), and the cfg-2 dimensions at B = 20 (R = 1024, a second column tile with four live columns, layer 0
from the gate table)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle import cases
from oracle import vog_oracle as vo
from tests.gpu_util import L, comm_for, engine_mod, flat, oracle_run, trace
from tests.test_gpu_forward import _OracleGolden, _check_against

pytestmark = pytest.mark.gpu
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
synth = importlib.import_module("vognet-pytorch_amd.synth")

SPECS = {
    "small_spat_b32": dict(over={"mdl.name": "vog", "ds.conc_type": "spat", **cases.REL, **cases.SMALL_DIMS}, B=32, vocab=50, dseed=81),
    "small_sep_b8": dict(over={"mdl.name": "vog", "ds.conc_type": "sep", **cases.REL, **cases.SMALL_DIMS}, B=8, vocab=50, dseed=82),
    "cfg2_b20": dict(over={"mdl.name": "vog", "ds.conc_type": "spat", **cases.REL}, B=20, vocab=5000, dseed=83),
}
_BUILT = {}


def make_batch(spec, B=None, dseed=None):
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, dict(spec["over"]))
    return synth.make_batch(cfg.ds.conc_type, B or spec["B"], 5, ncmp=4, vocab_size=spec["vocab"], prop_dim=cfg.mdl.prop_feat_dim,
                            seg_dim=cfg.mdl.seg_feat_dim, seed=dseed or spec["dseed"], ragged=True)


def built(key):
    """-> (engine with every option at its default, cfg, sd, batch, c, oracle result of `batch`), once per session"""
    if key not in _BUILT:
        spec = SPECS[key]
        cfg = ec.get_default_cfg()
        ec.update_from_dict(cfg, dict(spec["over"]))
        c = {"vocab": spec["vocab"], "nppf0": 5}
        sd = synth.init_state_dict(cfg, spec["vocab"], seed=1, perturb_ln=True)
        batch = make_batch(spec)
        eng = engine_mod.VogEngine(cfg, comm_for(c))
        eng.load_state_dict(sd)
        _BUILT[key] = (eng, cfg, sd, batch, c, golden(cfg, sd, batch, c))
    eng = _BUILT[key][0]
    eng.set_option("lstm_wide", 0)
    eng.set_option("lstm_persistent", 1)
    return _BUILT[key]


def golden(cfg, sd, batch, c):
    o = oracle_run(cfg, sd, batch, c)
    keys = ("mdl_outs", "mdl_outs_eval", "scores", "boxes", "indexs", "vidf_outs", "fin_scores", "fin_scores_loss")
    return _OracleGolden({k: o[k].numpy() for k in keys if k in o})


def to_dev(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}


def sentences(batch):
    return batch["srl_arg_words_ind"].shape[0] * batch["srl_arg_words_ind"].shape[1]


def check(key, tag, eng, out, batch, g):
    ncmp = batch["new_srl_idxs"].shape[1]
    assert bool(torch.isfinite(out["mdl_outs"]).all()), (key, tag)
    _check_against(f"{key}/{tag}", out, eng.unpack_pred(out["pred_rec"], ncmp), g, None, tol_rel=1e-3, tol_logit=6e-3)


# ---- which launches ----------------------------------------------------------------------------------------------------------
def test_step_description_follows_the_option():
    eng, cfg, sd, batch, c, _ = built("small_spat_b32")
    spec = SPECS["small_spat_b32"]
    layers = int(eng.desc.rnn_layers)
    dev = {B: to_dev(make_batch(spec, B=B, dseed=90 + B)) for B in (16, 33)}
    dev[32] = to_dev(batch)

    def steps(B):
        T = int(dev[B]["srl_arg_word_mask_len"].max())
        return flat(trace(eng, dev[B], None)), T

    off32, T32 = steps(32)
    off16, _ = steps(16)
    assert off32.count("lstm_layer") == 0 and off32.count("lstm_step") == layers * T32          # as before this option existed
    assert off16.count("lstm_layer") == layers and "lstm_step" not in off16
    eng.set_option("lstm_wide", 1)
    on32, _ = steps(32)
    assert on32.count("lstm_layer") == layers and "lstm_step" not in on32
    # everything but the recurrence is the option-off chain: the same steps (the pair pass places the visual ones elsewhere)
    strip = lambda tr: [n for n in tr if n not in ("lstm_layer", "lstm_step")]                   # noqa: E731
    assert sorted(strip(on32)) == sorted(strip(off32))
    assert not any("+" in n for n in trace(eng, dev[32], None)), "a wide layer is launched alone: no pair launches in its forward"
    on33, T33 = steps(33)
    assert on33.count("lstm_layer") == 0 and on33.count("lstm_step") == layers * T33
    # 16 sentences: the narrow kernel's ground - exactly the option-off description, pair launches included
    on16 = trace(eng, dev[16], None)
    eng.set_option("lstm_wide", 0)
    assert on16 == trace(eng, dev[16], None)
    # lstm_persistent = 0 switches the wide form off as well
    eng.set_option("lstm_wide", 1)
    eng.set_option("lstm_persistent", 0)
    deg, _ = steps(32)
    assert deg.count("lstm_layer") == 0 and deg.count("lstm_step") == layers * T32


def test_engine_applies_the_cfg_switch():
    spec = SPECS["small_spat_b32"]
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {**spec["over"], "hip.lstm_wide": True})
    _, _, sd, batch, c, _ = built("small_spat_b32")
    eng = engine_mod.VogEngine(cfg, comm_for(c))
    eng.load_state_dict(sd)
    tr = flat(trace(eng, to_dev(batch), None))
    assert "lstm_layer" in tr and "lstm_step" not in tr
    with pytest.raises(L.VogError):
        eng.set_option("lstm_wider", 1)


# ---- the whole forward against the CPU oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SPECS))
def test_forward_wide_vs_oracle(key):
    """eager forward with the option on; then the degrade path (lstm_persistent = 0: the step form) on the same batch"""
    eng, cfg, sd, batch, c, g = built(key)
    assert 17 <= sentences(batch) <= 32
    dev = to_dev(batch)
    before = {k: v.clone() for k, v in dev.items()}
    eng.set_option("lstm_wide", 1)
    tr = flat(trace(eng, dev, None))
    assert tr.count("lstm_layer") == int(eng.desc.rnn_layers) and "lstm_step" not in tr
    out = eng.forward(dev)
    torch.cuda.synchronize()
    eng.check()                                                  # no hand-off stalled
    for k in before:
        assert torch.equal(before[k], dev[k]), k
    check(key, "wide", eng, out, batch, g)
    wide_logits = out["mdl_outs"].clone()
    eng.set_option("lstm_persistent", 0)
    assert "lstm_layer" not in flat(trace(eng, dev, None))
    out = eng.forward(dev)
    torch.cuda.synchronize()
    check(key, "degraded to the step form", eng, out, batch, g)
    # (two faithful forms of one recurrence: another fp32 summation order, as test_forward_persistent_lstm_layer allows)
    assert (out["mdl_outs"] - wide_logits).abs().max().item() < 1.5e-3


@pytest.mark.parametrize("key", list(SPECS))
def test_slot_replay_wide_on_changed_inputs(key):
    """a captured slot launched twice on changed inputs: each replay equals the eager forward on the same data bit for bit (a
    stale hand-off slot surviving the previous replay would show here) and meets the oracle bound"""
    eng, cfg, sd, batch_a, c, g_a = built(key)
    batch_b = make_batch(SPECS[key], dseed=SPECS[key]["dseed"] + 40)
    g_b = golden(cfg, sd, batch_b, c)
    T = int(max(batch_a["srl_arg_word_mask_len"].max(), batch_b["srl_arg_word_mask_len"].max()))
    eng.set_option("lstm_wide", 1)
    slot = eng.make_slot(to_dev(batch_a), T=T, graph=True)
    keys = ("mdl_outs", "mdl_outs_eval", "pred_rec")
    for tag, batch, g in (("A", batch_a, g_a), ("B", batch_b, g_b), ("A again", batch_a, g_a)):
        if tag != "A":
            slot.update_inputs({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()})
        out = slot.launch()
        torch.cuda.synchronize()
        slot.check()
        got = {k: out[k].clone() for k in out if isinstance(out[k], torch.Tensor)}
        ref = eng.forward(to_dev(batch), T=T)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(got[k], ref[k]), (key, tag, k)
        check(key, f"slot {tag}", eng, got, batch, g)


@pytest.mark.parametrize("key", list(SPECS))
def test_bilstm_fwd_wide_vs_lstm_encoder(key):
    """vog_bilstm_fwd goes through the same builder: with the option on it runs the wide layers, against the oracle's
    restatement of the chain (lstm_encoder) within the bound of the narrow entry's test (4e-3: f16 operands, |h| < 1); padded
    outputs exactly 0 past each sentence's length"""
    eng, cfg, sd, batch, c, _ = built(key)
    eng.set_option("lstm_wide", 1)
    dev = to_dev(batch)
    b, out, (B, ncmp, T) = eng.make_batch(dev)
    lib = eng.lib
    n = lib.vog_lang_workspace_bytes(eng.ctx, B, ncmp, T)
    assert n > 0
    ws = torch.empty(int(n), dtype=torch.uint8, device="cuda")
    L.check(lib.vog_lang_workspace_init(eng.ctx, B, ncmp, T, ws.data_ptr(), ws.numel(), L.stream_ptr()), "init")
    assert flat(eng.describe_steps(b, ws, lang_only=True)).count("lstm_layer") == int(eng.desc.rnn_layers)
    Bn, R = sentences(batch), int(cfg.mdl.rnn.rnn_size)
    x = torch.full((Bn, T, 2 * R), float("nan"), device="cuda")
    fin = torch.full((Bn, 2 * R), float("nan"), device="cuda")
    for _ in range(2):                                                  # a second call on the same workspace: idempotent
        L.check(lib.vog_bilstm_fwd(eng.ctx, ctypes.byref(b), ws.data_ptr(), ws.numel(), x.data_ptr(), fin.data_ptr(), L.stream_ptr()),
                "vog_bilstm_fwd")
    torch.cuda.synchronize()
    eng.check()
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    inp = vo.to_torch(batch)
    lens = inp["srl_arg_word_mask_len"].reshape(-1)
    with torch.no_grad():
        tok = vo.srl_arg_seq_to_sent_seq(inp["srl_arg_words_ind"], inp["srl_arg_word_mask"], oc.vocab_size)
        xr, fr = vo.lstm_encoder(tok[:, :T].contiguous(), lens, vo.to_torch(sd), oc.rnn_layers)
    xg, fg = x.cpu(), fin.cpu()
    assert torch.isfinite(xg).all() and torch.isfinite(fg).all()
    for bi in range(Bn):
        assert (xg[bi, int(lens[bi]):] == 0).all()
    ex, ef = (xg - xr).abs().max().item(), (fg - fr).abs().max().item()
    print(key, "vog_bilstm_fwd (wide): x abs err", ex, "final hidden abs err", ef)
    assert ex < 4e-3 and ef < 4e-3
