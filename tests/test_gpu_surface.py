"""-m gpu: the DROP-IN SURFACE on hardware. Everything here goes through the reference's plugin
boundary - `get_mdl_loss_eval(cfg)` (code/mdl_selector.py:26-69) -> `cls(cfg, comm)`
(code/mdl_base.py:11-22) -> `load_state_dict` of a checkpoint-shaped dict -> `mdl(batch)` ->
`Evaluator*.get_out_results_boxes / forward_one_batch / forward` (code/eval_vsrl_corr.py) and the
`main_dist` CLI - never through VogEngine directly. Outputs are held to the same reference goldens
and tolerances as tests/test_gpu_forward.py."""
import importlib
import json
import pickle

import numpy as np
import pytest
import torch

from oracle import cases
from tests.gpu_util import comm_for
from tests.test_gpu_forward import _check_against

pytestmark = pytest.mark.gpu

sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
L = importlib.import_module("vognet-pytorch_amd.lib")
mgl = importlib.import_module("oracle.make_golden_loss")
synth = importlib.import_module("vognet-pytorch_amd.synth")

REF_RECORD_KEYS = {"pred_boxes", "pred_scores", "pred_cmp", "idx_vid", "idx_verbs", "idx_sent", "cmp_msk",
                   "targ_cmp", "perm", "perm_inv"}          # code/eval_vsrl_corr.py:247-273


def _meta(batch, seed=0):
    """The evaluator-side keys of a loader batch (dat_loader_simple.py:1476-1505)."""
    B, ncmp = batch["num_cmp_msk"].shape
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(ncmp) for _ in range(B)]).astype(np.int64)
    return {"ann_idx": np.arange(100, 100 + B, dtype=np.int64), "sent_idx": np.arange(7, 7 + B, dtype=np.int64),
            "target_cmp": rng.integers(0, ncmp, size=(B,)).astype(np.int64), "permute": perm,
            "permute_inv": np.argsort(perm, axis=1).astype(np.int64)}


def _build(name, key_style="module"):
    cfg, sd, batch, c = cases.build(name)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    comm = comm_for(c)
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    ck = {}
    for k, v in sd.items():
        kk = k
        if key_style == "ddp_tx" and (k.startswith("mult_txf.") or k.startswith("obj_txf.")):
            pre, rest = k.split(".", 1)                   # checkpoints of use_ddp=True transformers
            kk = f"{pre}.module.{rest}"
        if key_style in ("module", "ddp_tx"):
            kk = "module." + kk                           # DDP-wrapped model (trn_utils.py:536-592)
        if key_style == "legacy_ln" and "layernorm" in k:
            kk = k.replace(".weight", ".gamma").replace(".bias", ".beta")
        ck[kk] = torch.from_numpy(v)
    mdl.load_state_dict(ck)
    dev = {k: torch.from_numpy(v).cuda() for k, v in {**batch, **_meta(batch)}.items()}
    evl = sel["eval"](cfg, comm, torch.device("cuda", 0))
    return cfg, sel, mdl, evl, dev, batch, c


@pytest.mark.parametrize("name,key_style", [
    ("full/cfg2_vog_spat_gt5_bs4", "module"), ("full/cfg3_vog_temp_gt5_bs8", "ddp_tx"),
    ("full/vog_sep_gt5_bs4_ragged", "legacy_ln"), ("full/cfg5_vog_svsq_gt5_bs16", "plain"),
    ("small/vgrnd_temp", "module"), ("small/igrnd_sep", "module"), ("small/vog_spat_noobj", "ddp_tx")])
def test_selector_model_evaluator_vs_reference_golden(name, key_style):
    cfg, sel, mdl, evl, dev, batch, c = _build(name, key_style)
    before = {k: v.clone() for k, v in dev.items()}
    with torch.no_grad():
        out = mdl(dev)
    assert {"mdl_outs", "mdl_outs_eval"} <= set(out)
    if cfg.ds.conc_type in ("sep", "svsq"):
        assert {"vidf_outs", "fin_scores_loss", "fin_scores"} <= set(out)
    r = evl.get_out_results_boxes(out, dev)
    torch.cuda.synchronize()
    for k in before:
        assert torch.equal(before[k], dev[k]), k           # inputs are borrowed, never modified
    g = np.load(cases.golden_path(name))
    _check_against(name, out, r, g, None, tol_rel=1e-3, tol_logit=6e-3)
    # python-list records in the reference's format
    recs = evl.forward_one_batch(out, dev)
    B = batch["num_cmp_msk"].shape[0]
    assert len(recs) == B and set(recs[0]) == REF_RECORD_KEYS
    assert np.allclose(np.array(recs[1 % B]["pred_scores"]), g["scores"][1 % B], rtol=2e-3, atol=1e-6)
    assert recs[0]["idx_vid"] == 100 and recs[0]["perm"] == dev["permute"][0].tolist()


def test_inplace_weight_update_reaches_the_engine():
    """Parameters changed in place (optimizer.step / p.data.copy_) must not leave stale device weights."""
    cfg, sel, mdl, evl, dev, batch, c = _build("small/vog_spat")
    with torch.no_grad():
        a = mdl(dev)["mdl_outs"].clone()
        w = dict(mdl.named_parameters())["lin2.2.bias"]
        w.add_(0.5)
        b = mdl(dev)["mdl_outs"]
    torch.cuda.synchronize()
    assert torch.allclose(b, a + 0.5, atol=1e-5)


def test_slot_guards():
    """A slot refuses sentences longer than the T it was captured with, and refuses to launch after the
    engine's weights were re-finalized (its graph points at freed buffers)."""
    cfg, sel, mdl, evl, dev, batch, c = _build("full/cfg2_ragged")
    eng = mdl.engine()
    T = int(batch["srl_arg_word_mask_len"].max())
    slot = eng.make_slot(dev, graph=True)
    slot.launch()
    torch.cuda.synchronize()
    longer = {"srl_arg_word_mask_len": torch.full_like(dev["srl_arg_word_mask_len"], T + 1)}
    with pytest.raises(ValueError):
        slot.update_inputs(longer)
    slot.update_inputs({"srl_arg_word_mask_len": dev["srl_arg_word_mask_len"]})
    eng.load_state_dict(mdl.state_dict())
    with pytest.raises(Exception):
        slot.launch()


def test_two_streams_do_not_share_a_workspace():
    cfg, sel, mdl, evl, dev, batch, c = _build("full/cfg2_vog_spat_gt5_bs4")
    eng = mdl.engine()
    ref = eng.forward(dev)["mdl_outs"].clone()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(6):
        for st in (s1, s2):
            with torch.cuda.stream(st):
                outs.append(eng.forward(dev)["mdl_outs"])
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, ref)


class _Loader(list):
    pass


def test_evaluator_forward_loop_and_pickle(tmp_path):
    """Evaluator.forward: loop a loader, records through the ring exchange, rank 0 writes the pickle in the
    reference format (code/eval_vsrl_corr.py:101-150, 247-273); loss dict from the device loss."""
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    loss_fn = sel["loss"](cfg, comm_for(c))
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    cpu = {k: v.cpu() for k, v in dev.items()}
    cpu.update({k: torch.from_numpy(v) for k, v in tg.items()})
    dl = _Loader([cpu, cpu, cpu])
    val_loss, val_acc = evl(mdl, loss_fn, dl, "valid", rank=0, pred_path=tmp_path)
    assert set(val_acc) == set(evl.met_keys) and set(val_loss) == set(loss_fn.loss_keys)
    gl = np.load(mgl.loss_path(name))
    assert abs(float(val_loss["loss"]) - float(gl["loss"])) <= 2e-3 * float(gl["loss"])
    raw = open(tmp_path / "valid_0.pkl", "rb").read()
    recs = pickle.loads(raw)
    B = batch["num_cmp_msk"].shape[0]
    assert len(recs) == 3 * B and set(recs[0]) == REF_RECORD_KEYS
    # the file is what the reference's `pickle.dump(list of per-query dicts of Python lists)` writes, byte for byte (the
    # evaluator never builds the lists: fast_pickle.dumps_records; format pinned in tests/test_fast_pickle.py)
    assert pickle.dumps(recs, protocol=4) == raw
    assert list(recs[0]) == ["pred_boxes", "pred_scores", "pred_cmp", "idx_vid", "idx_verbs", "idx_sent", "cmp_msk", "targ_cmp",
                             "perm", "perm_inv"]
    assert isinstance(recs[0]["pred_boxes"][0][0][0][0], float) and isinstance(recs[0]["idx_vid"], int)
    g = np.load(cases.golden_path(name))
    for k in range(3):                                         # every batch, in loader order
        got = np.array([r["pred_scores"] for r in recs[k * B:(k + 1) * B]])
        assert np.allclose(got, g["scores"], rtol=2e-3, atol=1e-6)
        assert [r["idx_vid"] for r in recs[k * B:(k + 1) * B]] == list(range(100, 100 + B))


def test_evaluator_forward_scores_its_pickle_with_the_grounding_metrics(tmp_path):
    """With annotation files in cfg.ds the evaluator builds GroundEval_SPAT (eval_fn_corr.py) itself and
    `forward` returns the four metrics computed from the records the DEVICE produced: records -> ring ->
    pickle -> metrics, the reference's validation flow (code/eval_vsrl_corr.py:101-150)."""
    import pandas as pd
    from oracle import make_golden_metrics as G
    M = importlib.import_module("vognet-pytorch_amd.eval_fn_corr")
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sd, batch, c = cases.build(name)
    B, ncmp = batch["num_cmp_msk"].shape
    rows, ent = G.annotation_set(5, n_sent=40)
    sent = [8, 13, 21, 30][:B]
    for i, r in enumerate(rows):
        r["vt_split"] = "val" if i in sent else "test"
    pd.DataFrame(rows).to_csv(tmp_path / "srl.csv", index=False)
    pd.DataFrame({"dummy": [0]}).to_csv(tmp_path / "ann.csv", index=False)
    json.dump(ent, open(tmp_path / "ent.json", "w"))
    cfg.ds.val_ds4_inds, cfg.ds.val_ann_file = str(tmp_path / "srl.csv"), str(tmp_path / "ann.csv")
    cfg.ds.anet_ent_annot_file = str(tmp_path / "ent.json")
    sel = sel_mod.get_mdl_loss_eval(cfg)
    comm = comm_for(c)
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    evl = sel["eval"](cfg, comm, torch.device("cuda", 0))
    assert isinstance(evl.grnd_eval, M.GroundEval_SPAT)
    meta = _meta(batch)
    meta["sent_idx"] = np.array(sent, dtype=np.int64)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])     # (brings its own target_cmp)
    cpu = {k: torch.from_numpy(v) for k, v in {**batch, **meta, **tg}.items()}
    verbs = np.array([[1, 2, 3, 4]] * B, dtype=np.int64)
    verbs[np.arange(B), cpu["target_cmp"].numpy()] = meta["sent_idx"]
    cpu["new_srl_idxs"] = torch.from_numpy(verbs)
    loss_fn = sel["loss"](cfg, comm)
    val_loss, val_acc = evl(mdl, loss_fn, _Loader([cpu]), "valid", rank=0, pred_path=tmp_path)
    assert set(val_acc) == {"avg1", "avg1_cons", "avg1_vidf", "avg1_strict"}
    again = evl.grnd_eval.eval_ground_acc(tmp_path / "valid_0.pkl")
    for k, v in val_acc.items():
        assert 0.0 <= float(v) <= 1.0 and float(v) == pytest.approx(float(again[k]))
    assert again["num_queries"] == B                           # every validation sentence was scored


def test_main_dist_cli_only_val(capsys, tmp_path):
    """`main_dist.py <uid> --only_val=True --a.b=c`: the reference's CLI shape AND flow (code/main_dist.py:90-163
    -> Learner.validate, utils/trn_utils.py:443-468): the evaluator is called with (mdl, loss_fn, dl, dl_name,
    rank, pred_path), prints val_loss / val_acc and leaves `<tmp_path>/predictions/<uid>/valid_0.pkl` behind -
    with a short tail batch, as a drop_last=False validation loader produces."""
    main_mod.main_dist("t0", only_val=True, synthetic_batches=3,
                       **{"mdl.name": "vog", "ds.conc_type": "spat", "mdl.obj_tx.use_rel": True,
                          "mdl.mul_tx.use_rel": True, "train.bsv": 4, "misc.tmp_path": str(tmp_path)})
    lines = capsys.readouterr().out.splitlines()
    res = json.loads([l for l in lines if l.startswith("{\"uid\"")][-1])
    assert res["uid"] == "t0" and res["queries"] == 11 and res["mdl"] == "vog" and res["dl_name"] == "valid"
    assert set(res["val_loss"]) == {"loss", "mdl_out_loss"} and all(np.isfinite(v) and v > 0 for v in res["val_loss"].values())
    assert set(res["val_acc"]) == {"avg1", "avg1_cons", "avg1_vidf", "avg1_strict"}
    pk = tmp_path / "predictions" / "t0" / "valid_0.pkl"
    assert res["pred_file"] == str(pk) and pk.is_file()
    recs = pickle.load(open(pk, "rb"))
    assert len(recs) == 11 and set(recs[0]) == REF_RECORD_KEYS             # 4 + 4 + 3: the tail batch is short
    assert [r["idx_vid"] for r in recs] == list(range(11))                  # loader order, padding rows dropped
    with pytest.raises(AssertionError):
        main_mod.main_dist("t1", only_val=True, **{"mdl.no_such_key": 1})


def test_evaluator_forward_short_tail_batch(tmp_path):
    """The last batch of a validation loader is usually smaller (drop_last=False, utils/trn_utils.py:200-203):
    its records are padded to the exchange ring's row count and the padding is dropped again on rank 0."""
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    loss_fn = sel["loss"](cfg, comm_for(c))
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    cpu = {k: v.cpu() for k, v in dev.items()}
    cpu.update({k: torch.from_numpy(v) for k, v in tg.items()})
    B = batch["num_cmp_msk"].shape[0]
    tail = {k: v[: B - 1] for k, v in cpu.items()}
    val_loss, val_acc = evl(mdl, loss_fn, _Loader([cpu, cpu, tail]), "valid", rank=0, pred_path=tmp_path)
    recs = pickle.load(open(tmp_path / "valid_0.pkl", "rb"))
    assert len(recs) == 3 * B - 1
    g = np.load(cases.golden_path(name))
    got = np.array([r["pred_scores"] for r in recs[2 * B:]])
    assert np.allclose(got, g["scores"][: B - 1], rtol=2e-3, atol=1e-6)
    assert [r["idx_vid"] for r in recs[2 * B:]] == list(range(100, 100 + B - 1))
    assert set(val_loss) == set(loss_fn.loss_keys) and all(torch.isfinite(v) for v in val_loss.values())


# ---- device loss (csrc/loss.hip) through the selector's loss class -----------------------------------------
@pytest.mark.parametrize("name", mgl.LOSS_CASES)
def test_device_loss_vs_reference_golden(name):
    """LossB_* on the device against the goldens of the REFERENCE loss classes, fed with the reference's
    own forward outputs (isolates the loss): <= 2e-5 relative (fp32 summation order only)."""
    cfg, batch, c, tg = mgl.targets_for(name)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    loss_fn = sel["loss"](cfg, comm_for(c))
    g = np.load(cases.golden_path(name))
    gl = np.load(mgl.loss_path(name))
    out = {k: torch.from_numpy(g[k]).cuda() for k in ("mdl_outs", "vidf_outs") if k in g.files}
    inp = {k: torch.from_numpy(v).cuda() for k, v in {**batch, **tg}.items()}
    res = loss_fn(out, inp)
    torch.cuda.synchronize()
    assert {k for k in res if not k.startswith("_")} == set(gl.files) - {"sha_targets"} == set(loss_fn.loss_keys)
    for k in loss_fn.loss_keys:
        got, ref = float(res[k]), float(gl[k])
        assert abs(got - ref) <= 2e-5 * abs(ref), (k, got, ref)
    # bit-reproducible (fixed-order reduction)
    res2 = loss_fn(out, inp)
    assert all(torch.equal(res[k], res2[k]) for k in loss_fn.loss_keys)


@pytest.mark.parametrize("name", mgl.LOSS_CASES)
def test_device_loss_gradient_vs_reference_autograd(name):
    """LossB_*.backward (vog_loss_bwd): d loss / d mdl_outs - and d verb_loss / d vidf_outs for sep - against
    torch autograd through the REFERENCE loss classes (oracle/make_golden_loss.py::make_grad), fed with the
    reference's own forward outputs: <= 1e-6 abs (gradients are O(1e-2)), exactly 0 where the reference's is."""
    cfg, batch, c, tg = mgl.targets_for(name)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    loss_fn = sel["loss"](cfg, comm_for(c))
    g = np.load(cases.golden_path(name))
    gg = np.load(mgl.grad_path(name))
    out = {k: torch.from_numpy(g[k]).cuda() for k in ("mdl_outs", "vidf_outs") if k in g.files}
    inp = {k: torch.from_numpy(v).cuda() for k, v in {**batch, **tg}.items()}
    res = loss_fn(out, inp)
    sep = "grad_vidf_outs" in gg.files
    got = loss_fn.backward(res, with_verb=sep)
    torch.cuda.synchronize()
    gm = (got[0] if sep else got).cpu().numpy()
    ref = gg["grad_mdl_outs"]
    assert gm.shape == ref.shape
    assert np.abs(gm - ref).max() <= 1e-6 + 2e-5 * np.abs(ref).max(), np.abs(gm - ref).max()
    assert np.all(gm[ref == 0] == 0)
    if sep:
        gv = got[1].cpu().numpy()
        assert np.abs(gv - gg["grad_vidf_outs"]).max() <= 1e-6 + 2e-5 * np.abs(gg["grad_vidf_outs"]).max()


@pytest.mark.parametrize("name", ["full/cfg2_vog_spat_gt5_bs4", "full/cfg3_vog_temp_gt5_bs8",
                                  "full/vog_sep_gt5_bs4_ragged"])
def test_forward_then_loss_end_to_end(name):
    """mdl(batch) -> loss_fn(out, batch) entirely on the device vs the reference loss of the reference
    forward: the 16-bit forward moves logits by <= 6e-3, the loss (a mean of 4000 BCE terms) by <= 2e-3 rel."""
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    loss_fn = sel["loss"](cfg, comm_for(c))
    with torch.no_grad():
        res = loss_fn(mdl(dev), dev)
    gl = np.load(mgl.loss_path(name))
    for k in loss_fn.loss_keys:
        assert abs(float(res[k]) - float(gl[k])) <= 2e-3 * abs(float(gl[k])), (k, float(res[k]), float(gl[k]))


# ---- device-side SPAT / TEMP batch assembly (csrc/assemble.hip) ----------------------------------------------
mga = importlib.import_module("oracle.make_golden_assemble")
dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
vo = importlib.import_module("oracle.vog_oracle")


def _asm_cfg(conc):
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"ds.conc_type": conc})
    return cfg


@pytest.mark.parametrize("conc", ["spat", "temp"])
def test_device_assembly_vs_reference_fixture(conc):
    """Bit-exact against the output of the reference loader methods (tests/golden/assemble__*.npz)."""
    it = mga.items()
    g = np.load(mga.path(conc))
    asm = dls.DeviceBatchAssembler(_asm_cfg(conc), {"num_prop_per_frm": mga.SHAPE["nppf0"]})
    res = asm({k: torch.from_numpy(v).cuda() for k, v in it.items()})
    torch.cuda.synchronize()
    for k in mga.KEYS:
        got = res[k].cpu().numpy()
        assert got.shape == g[k].shape, k
        assert np.array_equal(got, g[k].astype(got.dtype)), k


@pytest.mark.parametrize("conc", ["spat", "temp"])
def test_device_assembly_full_size_into_slot_buffers(conc):
    """cfg-2 / cfg-3 sized items assembled straight into a slot's input tensors == the oracle's assembly, and
    the forward then runs on them (finite outputs)."""
    name = {"spat": "full/cfg2_vog_spat_gt5_bs4", "temp": "full/cfg3_vog_temp_gt5_bs8"}[conc]
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    B = batch["num_cmp_msk"].shape[0]
    it = synth.make_items(B, 4, c["nppf0"], seed=9)
    ref = vo.assemble_batch(it, conc, 10, c["nppf0"])
    asm = dls.DeviceBatchAssembler(cfg, comm_for(c))
    slot = mdl.engine().make_slot(dev, graph=True)
    asm({k: torch.from_numpy(v).cuda() for k, v in it.items()}, out={k: slot.inp[k] for k in dls.FWD_KEYS},
        with_loss_keys=False)
    out = slot.launch()
    torch.cuda.synchronize()
    for k in dls.FWD_KEYS:
        assert np.array_equal(slot.inp[k].cpu().numpy(), ref[k]), k
    assert torch.isfinite(out["mdl_outs"]).all()


# ---- backward, first slice (csrc/train_tx.hip): score head + the last mul_tx layer's tail ---------------------------
mgb = importlib.import_module("oracle.make_golden_bwd")
bwd = importlib.import_module("vognet-pytorch_amd.backward")


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "full/cfg2_vog_spat_gt5_bs4"])
def test_device_tail_backward_vs_reference_autograd(name):
    """loss -> d mdl_outs (`LossB_*.backward`, vog_loss_bwd) -> `vog_mul_tail_bwd`: the gradients of lin2 and of
    the last mul_tx layer's Wo / LayerNorm / FFN parameters and of the tail's two inputs, against AUTOGRAD THROUGH
    THE REFERENCE model + loss (tests/golden/bwd__*.npz). The tail's inputs (concatenated heads, layer input) come
    from the CPU oracle's fp32 forward (the 16-bit forward kernels keep no activations); the logits the loss
    gradient starts from are the reference's. Bound: 1e-3 of the largest reference entry per tensor (fp32 math on
    the fp32 matrix pipe: measured ~1e-5)."""
    from tests.test_bwd_oracle import check_fixture
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    g = np.load(mgb.bwd_path(name))
    layer = int(g["layer"])
    # the tail's inputs: oracle forward (CPU fp32, == reference to 4e-7)
    _, sd, _, _ = cases.build(name)
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    with torch.no_grad():
        o = vo.forward(oc, vo.to_torch(sd), vo.to_torch(batch), keep_stages=True)
    st = o["stages"]
    d = st["mul_tail_attn"].shape[-1]
    attn = st["mul_tail_attn"].reshape(-1, d).contiguous().cuda()
    x = st["mul_tail_x"].reshape(-1, d).contiguous().cuda()
    # d loss / d mdl_outs from the device loss on the reference's logits
    ref = np.load(cases.golden_path(name))
    out = {"mdl_outs": torch.from_numpy(ref["mdl_outs"]).cuda()}
    loss_fn = sel["loss"](cfg, comm_for(c))
    with torch.no_grad():
        ld = loss_fn(out, dev)
        assert abs(float(ld["loss"]) - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
        d_outs = loss_fn.backward(ld)
    B, nc_v, nsrl, NP = ref["mdl_outs"].shape
    nfrm = 40 if cfg.ds.conc_type == "temp" else 10
    nppf = NP // nfrm
    res = bwd.mul_tail_backward(sd_torch(sd), layer, attn, x, d_outs, B * nc_v, nfrm, nppf, nsrl)
    torch.cuda.synchronize()
    worst = 0.0
    for k, n in mgb.param_names(layer).items():
        worst = max(worst, check_fixture(g, k, res[n].cpu().numpy(), tol=1e-3))
    worst = max(worst, check_fixture(g, "d_attn", res["_d_attn"].cpu().numpy(), tol=1e-3))
    worst = max(worst, check_fixture(g, "d_x", res["_d_x"].cpu().numpy(), tol=1e-3))
    print(name, "worst relative gradient error", worst)
    assert worst <= 1e-3


def sd_torch(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _bwd_setup(name):
    """Oracle fp32 forward (activations at the seams), the device loss gradient on the reference's logits."""
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    g = np.load(mgb.bwd_path(name))
    _, sd, _, _ = cases.build(name)
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    with torch.no_grad():
        o = vo.forward(oc, vo.to_torch(sd), vo.to_torch(batch), keep_stages=True)
    ref = np.load(cases.golden_path(name))
    out = {"mdl_outs": torch.from_numpy(ref["mdl_outs"]).cuda()}
    loss_fn = sel["loss"](cfg, comm_for(c))
    with torch.no_grad():
        ld = loss_fn(out, dev)
        d_outs = loss_fn.backward(ld)
    B, nc_v, nsrl, NP = ref["mdl_outs"].shape
    nfrm = 40 if cfg.ds.conc_type == "temp" else 10
    return cfg, oc, sd, batch, g, o["stages"], d_outs, (B, nc_v, nsrl, NP, nfrm, NP // nfrm)


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "full/cfg2_vog_spat_gt5_bs4"])
def test_device_mul_layer_backward_vs_reference_autograd(name):
    """The whole last mul_tx layer + score head on the device (`encoder_layer_backward`: attention forward
    recomputation -> tail backward -> attention / QKV / box-bias backward, fp32): every parameter gradient of the
    layer, of `lin2` and of `pe_mul_sub_enc`, and the gradient of the layer input, against AUTOGRAD THROUGH THE
    REFERENCE model + loss. The layer input comes from the CPU oracle's forward."""
    from tests.test_bwd_oracle import check_fixture
    cfg, oc, sd, batch, g, st, d_outs, (B, nc_v, nsrl, NP, nfrm, nppf) = _bwd_setup(name)
    layer = int(g["layer"])
    d = st["mul_tail_x"].shape[-1]
    x = st["mul_tail_x"].reshape(-1, d).contiguous().cuda()
    S, N = B * nc_v * nfrm, nsrl * nppf
    boxes = None
    if oc.mul_use_rel:
        props = torch.from_numpy(batch["pad_proposals"]).float().reshape(-1, batch["pad_proposals"].shape[-1]).cuda()
        boxes = bwd._Boxes(props, oc.vid_w, oc.vid_h, float(nfrm))
    # the forward recomputation first: the device's fp32 layer output against the oracle's
    y, cat = bwd.encoder_layer_forward(sd_torch(sd), "mult_txf", layer, "pe_mul_sub_enc.0", x, S, N, nppf, oc.mul_heads, boxes)
    torch.cuda.synchronize()
    ref_cat = st["mul_tail_attn"].reshape(-1, d)
    assert float((cat.cpu() - ref_cat).abs().max()) <= 1e-4 * float(ref_cat.abs().max())
    ref_y = st["mul_out"].reshape(-1, d)
    assert float((y.cpu() - ref_y).abs().max()) <= 1e-4 * float(ref_y.abs().max())
    res = bwd.encoder_layer_backward(sd_torch(sd), "mult_txf", layer, "pe_mul_sub_enc.0", x, S, N, nppf, oc.mul_heads, boxes,
                                     head=(d_outs, B * nc_v, nfrm, nppf, nsrl))
    torch.cuda.synchronize()
    worst = 0.0
    names = list(bwd.layer_param_names("mult_txf", layer).values()) + ["lin2.0.weight", "lin2.0.bias", "lin2.2.weight", "lin2.2.bias"]
    if boxes is not None:
        names += ["pe_mul_sub_enc.0.weight", "pe_mul_sub_enc.0.bias"]
    for n in names:
        worst = max(worst, check_fixture(g, "p:" + n, res[n].cpu().numpy(), tol=1e-3))
    worst = max(worst, check_fixture(g, "d_mul_in", res["_d_x"].cpu().numpy(), tol=1e-3))
    print(name, "worst relative gradient error", worst)


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "full/cfg2_vog_spat_gt5_bs4"])
def test_device_visual_backward_vs_reference_autograd(name):
    """lin2 <- mul_tx <- concat / regroup <- obj_tx <- prop / segment encoders, chained on the device from the loss
    gradient (`visual_backward`): every parameter gradient on that side (49 tensors at cfg 2) and the gradients at the
    seams against AUTOGRAD THROUGH THE REFERENCE. Only the forward activations at three places come from the CPU
    oracle (mul_tx input, obj_tx input, the raw features); all gradients are the device's."""
    from tests.test_bwd_oracle import check_fixture
    cfg, oc, sd, batch, g, st, d_outs, (B, nc_v, nsrl, NP, nfrm, nppf) = _bwd_setup(name)
    geo = dict(B=B, nc_v=nc_v, nfrm=nfrm, nppf=nppf, nsrl=nsrl, nppf0=oc.nppf0, mul_layers=oc.mul_layers, mul_heads=oc.mul_heads,
               mul_use_rel=oc.mul_use_rel, obj_layers=oc.obj_layers if (oc.mdl_name == "vgrnd" or oc.obj_to_use) else 0,
               obj_heads=oc.obj_heads, obj_use_rel=oc.obj_use_rel, obj_one_frm=oc.obj_one_frm, vid_w=oc.vid_w, vid_h=oc.vid_h)
    assert oc.mul_layers == 1 and geo["obj_layers"] == 1      # inner layer inputs would come from the device's own forward
    dm = st["mul_tail_x"].shape[-1]
    dobj = st["obj_tail_x"].shape[-1]
    acts = {"mul_x": st["mul_tail_x"].reshape(-1, dm).contiguous().cuda(),
            "obj_x": st["obj_tail_x"].reshape(-1, dobj).contiguous().cuda(),
            "prop_feat": torch.from_numpy(batch["pad_region_feature"]).float().reshape(-1, batch["pad_region_feature"].shape[-1]).cuda(),
            "seg_feat": torch.from_numpy(batch["seg_feature_for_frms"]).float().reshape(-1, batch["seg_feature_for_frms"].shape[-1]).cuda(),
            "props": torch.from_numpy(batch["pad_proposals"]).float().reshape(-1, batch["pad_proposals"].shape[-1]).cuda(),
            "inds_msk": torch.from_numpy(batch["srl_arg_inds_msk"]).cuda()}
    res = bwd.visual_backward(sd_torch(sd), geo, acts, d_outs)
    torch.cuda.synchronize()
    worst, n_par = 0.0, 0
    for k, v in res.items():
        if k.startswith("_"):
            continue
        worst = max(worst, check_fixture(g, "p:" + k, v.cpu().numpy(), tol=1e-3))
        n_par += 1
    assert n_par == 12 + 4 + 2 + 12 + 2 + 4, n_par
    worst = max(worst, check_fixture(g, "d_obj_out", res["_d_obj_out"].cpu().numpy(), tol=1e-3))
    worst = max(worst, check_fixture(g, "d_obj_in", res["_d_prop_seg"].cpu().numpy(), tol=1e-3))
    worst = max(worst, check_fixture(g, "d_lang_enc", res["_d_lang"].cpu().numpy(), tol=1e-3))
    print(name, "worst relative gradient error", worst, "parameters", n_par)


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "full/cfg2_vog_spat_gt5_bs4"])
def test_device_full_backward_vs_reference_autograd(name):
    """The whole network behind the loss on the device in fp32: `visual_backward` (lin2, mul_tx, obj_tx, encoders) and,
    from its gradient of the argument vectors, `language_backward` (srl_arg_words_out_enc, lstm_out_feat_proj, the
    packed 2-layer BiLSTM through time, the embedding): EVERY parameter the reference's loss.backward() reaches
    (59 tensors at cfg 2) against autograd through the reference model + loss. The language side recomputes its own
    forward on the device (checked against the oracle's argument vectors)."""
    from tests.test_bwd_oracle import check_fixture
    cfg, oc, sd, batch, g, st, d_outs, (B, nc_v, nsrl, NP, nfrm, nppf) = _bwd_setup(name)
    geo = dict(B=B, nc_v=nc_v, nfrm=nfrm, nppf=nppf, nsrl=nsrl, nppf0=oc.nppf0, mul_layers=oc.mul_layers, mul_heads=oc.mul_heads,
               mul_use_rel=oc.mul_use_rel, obj_layers=oc.obj_layers if (oc.mdl_name == "vgrnd" or oc.obj_to_use) else 0,
               obj_heads=oc.obj_heads, obj_use_rel=oc.obj_use_rel, obj_one_frm=oc.obj_one_frm, vid_w=oc.vid_w, vid_h=oc.vid_h)
    dm, dobj = st["mul_tail_x"].shape[-1], st["obj_tail_x"].shape[-1]
    acts = {"mul_x": st["mul_tail_x"].reshape(-1, dm).contiguous().cuda(),
            "obj_x": st["obj_tail_x"].reshape(-1, dobj).contiguous().cuda(),
            "prop_feat": torch.from_numpy(batch["pad_region_feature"]).float().reshape(-1, batch["pad_region_feature"].shape[-1]).cuda(),
            "seg_feat": torch.from_numpy(batch["seg_feature_for_frms"]).float().reshape(-1, batch["seg_feature_for_frms"].shape[-1]).cuda(),
            "props": torch.from_numpy(batch["pad_proposals"]).float().reshape(-1, batch["pad_proposals"].shape[-1]).cuda(),
            "inds_msk": torch.from_numpy(batch["srl_arg_inds_msk"]).cuda()}
    sdt = sd_torch(sd)
    res = bwd.visual_backward(sdt, geo, acts, d_outs)
    dev_batch = {k: torch.from_numpy(batch[k]).cuda() for k in ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len",
                                                                 "srl_arg_words_capture")}
    T = int(batch["srl_arg_word_mask_len"].max())
    lg = bwd.language_backward(sdt, dev_batch, T, oc.rnn_layers, d_lang_enc=res["_d_lang"])
    torch.cuda.synchronize()
    # the language side's own forward: argument vectors before the mask
    ref_le = st["lang_enc"].reshape(-1, st["lang_enc"].shape[-1])
    assert float((lg["_lang_enc"].cpu() - ref_le).abs().max()) <= 1e-4 * float(ref_le.abs().max())
    res.update(lg)
    worst, n_par = 0.0, 0
    have = {k[2:-len("__shape")] for k in g.files if k.startswith("p:") and k.endswith("__shape")}
    for k, v in res.items():
        if k.startswith("_"):
            continue
        worst = max(worst, check_fixture(g, "p:" + k, v.cpu().numpy(), tol=1e-3))
        n_par += 1
    missing = have - {k for k in res if not k.startswith("_")}
    assert not missing, missing
    print(name, "worst relative gradient error", worst, "parameters", n_par)


@pytest.mark.parametrize("name", ["small/vog_spat", "full/cfg2_vog_spat_gt5_bs4", "small/vog_sep_r64", "full/cfg5_vog_svsq_gt5_bs16",
                                  "small/igrnd_spat", "small/vgrnd_temp", "small/vgrnd_sep", "full/cfg1_igrnd_spat_gt5_bs2",
                                  "full/cfg2_ragged", "small/vog_sep_cmpmsk", "small/vog_spat_3layers", "small/vog_temp_objonefrm",
                                  "small/vog_spat_noobj", "small/vog_spat_norel",
                                  "full/vgrnd_spat_gt5_bs4", "full/vog_spat_gt5_bs4_3layers"])
def test_device_training_steps_vs_oracle_adam(name):
    """`FP32Trainer.step` x 3 on the device (fp32 forward with its own activations -> device loss -> loss gradient ->
    visual / language backward -> Adam, all C-ABI calls) against the same three steps on the CPU: autograd through
    the oracle forward + loss (== autograd through the reference, tests/test_bwd_oracle.py) and torch.optim.Adam
    with the reference's betas (0.9, 0.99) (code/main_dist.py:55). Compared: the loss of every step and every
    parameter after the last one."""
    trn = importlib.import_module("vognet-pytorch_amd.train")
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    _, sd, _, _ = cases.build(name)
    lr, steps = 1e-4, 3
    loss_fn = sel["loss"](cfg, comm_for(c))
    tr = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=lr)
    # the device's first-step gradients against the reference fixture (the forward here is the device's own)
    from tests.test_bwd_oracle import check_fixture
    g = np.load(mgb.bwd_path(name))
    ld, grads = tr.gradients(dev)
    assert abs(float(ld["loss"]) - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    # (bound 5e-3 here, 1e-3 where the activations are the oracle's: with the device's own fp32 forward a ReLU whose
    # pre-activation is ~1e-7 can land on the other side of zero, which moves one row's contribution to dW -
    # measured 9e-7 with the current summation order, 1.6e-3 with an earlier one)
    ref_outs = torch.from_numpy(np.load(cases.golden_path(name))["mdl_outs"])
    fo = tr.forward(dev)[0]
    outs = fo["mdl_outs"].cpu()
    assert float((outs - ref_outs).abs().max()) <= 1e-4 * float(ref_outs.abs().max())
    if "vidf_outs" in fo:                                   # sep / svsq: the verb head's logits (reported as verb_loss)
        ref_v = torch.from_numpy(np.load(cases.golden_path(name))["vidf_outs"])
        assert float((fo["vidf_outs"].cpu() - ref_v).abs().max()) <= 1e-4 * max(1.0, float(ref_v.abs().max()))
    worst = max(check_fixture(g, "p:" + k, v.cpu().numpy(), tol=5e-3) for k, v in grads.items())
    n_exp = sum(1 for k in g.files if k.startswith("p:") and k.endswith("__shape"))
    assert len(grads) == n_exp, (len(grads), n_exp)
    if "verb_loss" in ld:
        assert float(ld["verb_loss"]) > 0
    dev_losses = [float(tr.step(dev)["loss"]) for _ in range(steps)]
    torch.cuda.synchronize()
    # CPU: oracle autograd + torch Adam
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    sdt = {k: v.clone().requires_grad_(True) for k, v in vo.to_torch(sd).items()}
    inp = vo.to_torch({**batch, **tg})
    opt = torch.optim.Adam(list(sdt.values()), lr=lr, betas=(0.9, 0.99))
    torch.set_num_threads(8)
    cpu_losses = []
    for _ in range(steps):
        opt.zero_grad()
        res = vo.loss_forward(oc, vo.forward(oc, sdt, inp), inp, loss_lambda=float(cfg.loss.loss_lambda))
        res["loss"].backward()
        opt.step()
        cpu_losses.append(float(res["loss"].detach()))
    for a, b in zip(dev_losses, cpu_losses):
        assert abs(a - b) <= 1e-4 * abs(b), (dev_losses, cpu_losses)
    # parameters after 3 Adam steps: each step moves an entry by at most ~lr. Adam divides by sqrt(v): an entry whose
    # gradient is rounding noise around zero (1e-12 next to 1e-3) still moves by +-lr, with the noise's sign - those
    # entries (a fraction of a per cent: unused embedding columns, dead units) may differ by a full step, every other
    # entry agrees to a small fraction of lr
    after = tr.state_dict()
    bad, tot, worst_p = 0, 0, 0.0
    for k, v in sdt.items():
        if v.grad is None:
            assert torch.equal(after[k].cpu(), vo.to_torch(sd)[k]), k          # untouched parameters stay bit-identical
            continue
        diff = (after[k].cpu() - v.detach()).abs()
        worst_p = max(worst_p, float(diff.max()))
        bad += int((diff > 0.05 * lr).sum())
        tot += diff.numel()
    print(name, "first-step gradients", worst, "losses", dev_losses, cpu_losses, "max param diff / lr", worst_p / lr, "entries off by > 5% of lr:", bad, "of", tot)
    assert bad <= 5e-3 * tot and worst_p <= 2.0 * lr * steps


def test_main_dist_cli_fit(capsys, tmp_path):
    """`main_dist.py <uid> --a.b=c` without only_val: `Learner.fit` (code/main_dist.py:125, utils/trn_utils.py:701-775)
    - two epochs of the device training step over synthetic batches, the validation flow after each on the inference
    model with the new weights, the checkpoint in the reference's layout; the training loss falls, and a second run
    resumes from the checkpoint (model + optimizer)."""
    kw = {"mdl.name": "vog", "ds.conc_type": "spat", "mdl.obj_tx.use_rel": True, "mdl.mul_tx.use_rel": True,
          "train.bs": 4, "train.bsv": 4, "train.epochs": 2, "train.lr": 1e-4, "misc.tmp_path": str(tmp_path)}
    hist = main_mod.main_dist("f0", synthetic_batches=4, **kw)
    lines = capsys.readouterr().out.splitlines()
    res = json.loads([l for l in lines if l.startswith("{\"uid\"")][-1])
    assert res["epochs"] == 2 and res["train_steps"] == 8
    assert hist[1]["trn_loss"] < hist[0]["trn_loss"] and all(np.isfinite(list(h.values())).all() for h in hist)
    ck = torch.load(open(res["model_file"], "rb"), weights_only=False)
    assert {"model_state_dict", "optimizer_state_dict", "num_it", "num_epoch", "cfgtxt", "best_met"} <= set(ck)
    assert "lstm_encoder.lstm.weight_hh_l1_reverse" in ck["model_state_dict"] and len(ck["optimizer_state_dict"]["state"]) == 57
    # resume (model + optimizer state): the checkpoint is the best epoch's; resumed after epoch 1 the run replays epoch 2
    # and - every reduction on this path has a fixed order - reproduces its smoothed loss exactly
    hist2 = main_mod.main_dist("f0", synthetic_batches=4, **{**kw, "train.epochs": 1, "train.load_opt": True})
    if ck["num_epoch"] == 1:
        assert hist2[0]["trn_loss"] == hist[1]["trn_loss"]
    else:
        assert hist2[0]["trn_loss"] < hist[1]["trn_loss"]


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep_r64", "small/vgrnd_temp", "full/cfg2_vog_spat_gt5_bs4"])
def test_device_training_with_dropout_vs_oracle_with_the_same_masks(name):
    """Train mode: LSTMEncoder's dropouts (embeddings, between the layers, output), the transformers' attn_drop on the
    attention probabilities and on both sub-layer outputs - masks from the device's counter-based generator
    (csrc/train_dev.h::drop_scale, restated as oracle.drop_mask). The reference's masks come from torch's generator and
    cannot be reproduced by anything else; what is pinned here is that forward AND backward use the masks consistently:
    loss and all parameter gradients of one step equal autograd through the oracle run with the SAME masks, and two
    Adam steps (a new seed per step) follow it."""
    trn = importlib.import_module("vognet-pytorch_amd.train")
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    _, sd, _, _ = cases.build(name)
    lr = 1e-4
    loss_fn = sel["loss"](cfg, comm_for(c))
    tr = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=lr, dropout=True, dropout_seed=3)
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    inp = vo.to_torch({**batch, **tg})
    torch.set_num_threads(8)
    p_obj, p_mul = float(cfg.mdl.obj_tx.attn_drop), float(cfg.mdl.mul_tx.attn_drop)
    assert p_obj > 0 and p_mul > 0

    def cpu_grads(sdt, seed):
        res = vo.loss_forward(oc, vo.forward(oc, sdt, inp, drop=seed, p_obj=p_obj, p_mul=p_mul), inp,
                              loss_lambda=float(cfg.loss.loss_lambda))
        res["loss"].backward()
        return float(res["loss"].detach())

    # one step's loss and gradients, the masks of step 1
    sdt = {k: v.clone().requires_grad_(True) for k, v in vo.to_torch(sd).items()}
    l_cpu = cpu_grads(sdt, tr._step_seed())
    ld, grads = tr.gradients(dev)
    with torch.no_grad():                                   # dropout changes the loss visibly (it is really on)
        l_eval = float(vo.loss_forward(oc, vo.forward(oc, vo.to_torch(sd), inp), inp, loss_lambda=float(cfg.loss.loss_lambda))["loss"])
    assert abs(l_cpu - l_eval) > 1e-6 * abs(l_eval)          # (random-init logits are small: the loss moves in the 5th digit)
    assert abs(float(ld["loss"]) - l_cpu) <= 2e-5 * abs(l_cpu), (float(ld["loss"]), l_cpu)
    worst = 0.0
    for k, gdev in grads.items():
        ref = sdt[k].grad
        scale = max(float(ref.abs().max()), 1e-12)
        worst = max(worst, float((gdev.cpu() - ref).abs().max()) / scale)
    assert worst <= 5e-3, worst
    # two optimisation steps (seed changes per step) against torch Adam on the oracle
    sdt = {k: v.clone().requires_grad_(True) for k, v in vo.to_torch(sd).items()}
    opt = torch.optim.Adam(list(sdt.values()), lr=lr, betas=(0.9, 0.99))
    dl, cl = [], []
    for _ in range(2):
        opt.zero_grad()
        cl.append(cpu_grads(sdt, tr._step_seed()))
        opt.step()
        dl.append(float(tr.step(dev)["loss"]))
    for a, b in zip(dl, cl):
        assert abs(a - b) <= 1e-4 * abs(b), (dl, cl)
    print(name, "dropout step: loss", float(ld["loss"]), l_cpu, "(eval-mode loss", l_eval, ") worst gradient error", worst, "losses", dl, cl)


@pytest.mark.parametrize("name", ["small/vog_spat", "full/cfg2_vog_spat_gt5_bs4"])
def test_device_training_mixed_precision_close_to_fp32(name):
    """`bf16_gemm`: the tile GEMMs of the training path with bf16 operands (fp32 accumulation, fp32 master weights). Not the
    pinned path - a faster one: its loss equals the fp32 loss to 1e-3, every parameter gradient points the fp32 gradient's
    way (cosine >= 0.99, largest single deviation <= 0.2 of the tensor's largest entry), and three Adam steps track the fp32
    trainer's losses to 1e-2."""
    trn = importlib.import_module("vognet-pytorch_amd.train")
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    _, sd, _, _ = cases.build(name)
    loss_fn = sel["loss"](cfg, comm_for(c))
    t32 = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=1e-4)
    t16 = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=1e-4, bf16_gemm=True)
    l32, g32 = t32.gradients(dev)
    l16, g16 = t16.gradients(dev)
    assert abs(float(l16["loss"]) - float(l32["loss"])) <= 1e-3 * abs(float(l32["loss"]))
    worst = 0.0
    differs = False
    errs, cos_min = {}, 1.0
    for k in g32:
        scale = max(float(g32[k].abs().max()), 1e-12)
        e = float((g16[k] - g32[k]).abs().max()) / scale
        errs[k] = e
        worst = max(worst, e)
        differs |= e > 1e-6
        a64, b64 = g32[k].double().reshape(-1), g16[k].double().reshape(-1)
        if float(a64.norm()) > 0:
            cos_min = min(cos_min, float(a64 @ b64 / (a64.norm() * b64.norm())))
    print(sorted(errs.items(), key=lambda kv: -kv[1])[:4], "min cosine", cos_min)
    # the deviation grows with the depth of the backward chain behind a tensor (measured at cfg 2: 1e-2 for lin2 / mul_tx, 0.12
    # of the largest entry for the segment encoder's weight at the far end); directions agree
    assert differs and worst <= 0.2 and cos_min >= 0.99, (worst, cos_min)
    a = [float(t32.step(dev)["loss"]) for _ in range(3)]
    b = [float(t16.step(dev)["loss"]) for _ in range(3)]
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-2 * abs(x), (a, b)
    print(name, "bf16 GEMMs: worst gradient deviation", worst, "losses fp32", a, "bf16", b)


def test_learner_surface(tmp_path):
    """`trn_utils.Learner` with the reference's constructor and methods (utils/trn_utils.py:265-860): fit -> files in the
    reference's places (txt_logs / models / predictions), validate on a named loader, testing on a dict of loaders,
    save / load round trip (a fresh Learner resumes from the checkpoint: same parameters, same optimizer step)."""
    tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
    name = "small/vog_spat"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    comm = comm_for(c)
    cfg.defrost() if hasattr(cfg, "defrost") else None
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    B = batch["num_cmp_msk"].shape[0]
    ncmp = batch["num_cmp_msk"].shape[1]
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one, one, one], valid_dl=[one], test_dl=[one])
    loss_fn = sel["loss"](cfg, comm)
    learn = tu.Learner(uid="L0", data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)
    hist = learn.fit(epochs=2, lr=1e-4)
    assert len(hist) == 2 and hist[1]["trn_loss"] < hist[0]["trn_loss"] and learn.num_it == 6
    assert learn.model_file == tmp_path / "models" / "L0.pth" and learn.model_file.is_file()
    assert learn.txt_log_file.is_file() and "trn_loss" in learn.txt_log_file.read_text()
    assert (learn.predictions_dir / "valid_0.pkl").is_file()
    vl, va, _ = learn.validate({"mytest": [one]})
    assert (learn.predictions_dir / "mytest_0.pkl").is_file() and set(vl) == set(loss_fn.loss_keys) and set(va) == set(evl.met_keys)
    res = learn.testing({"t1": [one]})
    assert "t1" in res and (learn.predictions_dir / "t1_0.pkl").is_file()
    learn.save_model_dict()
    cfg2, sel2, mdl2, evl2, _, _, _ = _build(name)
    cfg2.train.load_opt = True if not getattr(cfg2, "is_frozen", lambda: False)() else cfg2.train.load_opt
    learn2 = tu.Learner(uid="L0", data=data, mdl=mdl2, loss_fn=sel2["loss"](cfg2, comm), cfg=cfg2, eval_fn=evl2, comm=comm)
    for k, v in learn.trainer.state_dict().items():
        assert torch.equal(v, learn2.trainer.params[k]), k
    assert learn2.num_epoch == learn.num_epoch
    assert learn2.trainer.num_it == 6 and learn2.trainer.adam_step == 6         # load_opt: Adam's step comes with m / v

    # resume WITHOUT the optimizer state (the reference's defaults: resume = True, load_opt = False, utils/trn_utils.py:594-605):
    # the Learner's iteration counter is restored, Adam starts fresh - step 0, m = v = 0. (a restored step count
    # against zero moments switched the bias correction off: first update ~3.2 x lr.) The first update after the resume must be
    # torch.optim.Adam's first update from that checkpoint.
    cfg3, sel3, mdl3, evl3, _, _, _ = _build(name)
    assert not cfg3.train.load_opt
    learn3 = tu.Learner(uid="L0", data=data, mdl=mdl3, loss_fn=sel3["loss"](cfg3, comm), cfg=cfg3, eval_fn=evl3, comm=comm)
    tr3 = learn3.trainer
    assert tr3.num_it == 6 and tr3.adam_step == 0 and not tr3.m
    before = {k: v.clone() for k, v in tr3.params.items()}
    dev_b = {k: v.cuda() for k, v in one.items()}
    _, grads = tr3.gradients(dev_b)
    grads = {k: v.clone() for k, v in grads.items()}
    tr3.step(dev_b)
    torch.cuda.synchronize()
    worst = 0.0
    for k, g in grads.items():
        p = torch.nn.Parameter(before[k].clone())
        opt = torch.optim.Adam([p], lr=tr3.lr, betas=tr3.betas, eps=tr3.eps)
        p.grad = g.clone()
        opt.step()
        upd_ref = (p.detach() - before[k])
        upd = tr3.params[k] - before[k]
        worst = max(worst, float((upd - upd_ref).abs().max()) / max(float(upd_ref.abs().max()), 1e-12))
    print("first update after a resume without optimizer state vs torch.optim.Adam: worst relative deviation", worst)
    assert worst < 1e-3, worst


def test_evaluator_batches_requests(capsys, tmp_path):
    """`cfg.hip.batch_requests = 4`: Evaluator.forward serves four loader batches as ONE forward (dynamic batching). Same
    records in the same order, the same per-batch-averaged loss as one forward per loader batch - incl. a short tail batch
    inside the last group."""
    kw = {"mdl.name": "vog", "ds.conc_type": "spat", "mdl.obj_tx.use_rel": True, "mdl.mul_tx.use_rel": True, "train.bsv": 4,
          "misc.tmp_path": str(tmp_path)}
    main_mod.main_dist("b1", only_val=True, synthetic_batches=6, **kw)
    r1 = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{\"uid\"")][-1])
    main_mod.main_dist("b4", only_val=True, synthetic_batches=6, **{**kw, "hip.batch_requests": 4})
    r4 = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{\"uid\"")][-1])
    assert r1["queries"] == r4["queries"] == 23
    for k in r1["val_loss"]:
        assert abs(r1["val_loss"][k] - r4["val_loss"][k]) <= 2e-4 * abs(r1["val_loss"][k]), (k, r1["val_loss"], r4["val_loss"])
    a = pickle.load(open(r1["pred_file"], "rb"))
    b = pickle.load(open(r4["pred_file"], "rb"))
    assert len(a) == len(b) == 23 and [x["idx_vid"] for x in a] == [x["idx_vid"] for x in b]
    for x, y in zip(a, b):
        assert np.abs(np.array(x["pred_scores"]) - np.array(y["pred_scores"])).max() <= 4e-4
        assert x["pred_cmp"] == y["pred_cmp"] or np.abs(np.array(x["pred_scores"])).max() > 0      # (ties aside, the same choices)


def test_two_trainers_with_different_gemm_settings_in_one_process():
    """`bf16_gemm` is not process state (round 3: a process-wide static in what is now csrc/train_gemm.hip): two trainers with different
    settings, called alternately, each reproduce what they compute alone, bit for bit (the training path has no atomics), the
    switch is off again behind every call, and another thread never sees this thread's choice."""
    import ctypes
    import threading
    trn = importlib.import_module("vognet-pytorch_amd.train")
    Lm = importlib.import_module("vognet-pytorch_amd.lib")
    name = "small/vog_spat"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    _, sd, _, _ = cases.build(name)
    loss_fn = sel["loss"](cfg, comm_for(c))
    t32 = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=1e-4)
    t16 = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=1e-4, bf16_gemm=True)
    _, a32 = t32.gradients(dev)
    _, a16 = t16.gradients(dev)
    a32 = {k: v.clone() for k, v in a32.items()}
    a16 = {k: v.clone() for k, v in a16.items()}
    assert any(not torch.equal(a32[k], a16[k]) for k in a32)           # the settings do differ in what they compute
    lib = Lm.load()

    def flag():
        v = ctypes.c_int32(-1)
        assert lib.vog_train_get_int(b"bf16_gemm", ctypes.byref(v)) == 0
        return v.value

    for _ in range(2):                                                  # alternating in one thread
        _, g16 = t16.gradients(dev)
        assert flag() == 0
        _, g32 = t32.gradients(dev)
        for k in a32:
            assert torch.equal(g32[k], a32[k]), k
            assert torch.equal(g16[k], a16[k]), k
    # a second thread does not see this thread's choice (the training path's Python-side scratch caches are per process and
    # single-threaded by contract - SURVEY 8(b) "single-threaded caller per process" - so trainers are not RUN concurrently)
    assert lib.vog_train_set_int(b"bf16_gemm", 1) == 0 and flag() == 1
    seen = {}
    th = threading.Thread(target=lambda: seen.update(other=flag()))
    th.start()
    th.join()
    assert seen == {"other": 0}
    assert lib.vog_train_set_int(b"bf16_gemm", 0) == 0 and flag() == 0


@pytest.mark.parametrize("name", ["full/cfg2_vog_spat_gt5_bs4", "full/cfg2_ragged", "small/vog_sep"])
def test_bilstm_fwd_entry_point_matches_oracle_lstm_encoder(name):
    """`vog_bilstm_fwd` (SURVEY 8(b) minimum export set): LSTMEncoder.forward on its own - re-index, embedding, both layers,
    both directions - against the oracle's `lstm_encoder` (utils/mdl_srl_utils.py:114-169): padded outputs exactly 0 past
    each sentence's length, final hidden = [h_fwd(last valid) || h_bwd(step 0)] of the top layer."""
    import ctypes
    from oracle import vog_oracle as vo
    eng_mod = importlib.import_module("vognet-pytorch_amd.engine")
    Lm = importlib.import_module("vognet-pytorch_amd.lib")
    cfg, sd, batch, c = cases.build(name)
    eng = eng_mod.VogEngine(cfg, comm_for(c))
    eng.load_state_dict(sd)
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    b, out, (B, ncmp, T) = eng.make_batch(dev)
    lib = eng.lib
    n = lib.vog_lang_workspace_bytes(eng.ctx, B, ncmp, T)
    assert n > 0
    ws = torch.empty(int(n), dtype=torch.uint8, device="cuda")
    Lm.check(lib.vog_lang_workspace_init(eng.ctx, B, ncmp, T, ws.data_ptr(), ws.numel(), Lm.stream_ptr()), "init")
    Bn = dev["srl_arg_words_ind"].shape[0] * dev["srl_arg_words_ind"].shape[1]
    R = cfg.mdl.rnn.rnn_size
    x = torch.full((Bn, T, 2 * R), float("nan"), device="cuda")
    fin = torch.full((Bn, 2 * R), float("nan"), device="cuda")
    for _ in range(2):                                                  # a second call on the same workspace: idempotent
        Lm.check(lib.vog_bilstm_fwd(eng.ctx, ctypes.byref(b), ws.data_ptr(), ws.numel(), x.data_ptr(), fin.data_ptr(),
                                    Lm.stream_ptr()), "vog_bilstm_fwd")
    torch.cuda.synchronize()
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    inp = vo.to_torch(batch)
    sdt = vo.to_torch(sd)
    lens = inp["srl_arg_word_mask_len"].reshape(-1)
    with torch.no_grad():
        tok = vo.srl_arg_seq_to_sent_seq(inp["srl_arg_words_ind"], inp["srl_arg_word_mask"], oc.vocab_size)
        xr, fr = vo.lstm_encoder(tok[:, :T].contiguous(), lens, sdt, oc.rnn_layers)
    xg, fg = x.cpu(), fin.cpu()
    assert torch.isfinite(xg).all() and torch.isfinite(fg).all()
    for bi in range(Bn):
        assert (xg[bi, int(lens[bi]):] == 0).all()
    ex, ef = (xg - xr).abs().max().item(), (fg - fr).abs().max().item()
    print(name, "vog_bilstm_fwd: x abs err", ex, "final hidden abs err", ef)
    assert ex < 4e-3 and ef < 4e-3            # f16 operands, fp32 cell state: |h| < 1


def test_optimizer_state_of_another_model_is_refused():
    """Adam state is mapped by position; a state whose shape is not its parameter's must raise instead of letting
    vog_adam_f32 walk a shorter m / v buffer. The repo's own checkpoint still round-trips."""
    trn = importlib.import_module("vognet-pytorch_amd.train")
    name = "small/vog_spat"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev.update({k: torch.from_numpy(v).cuda() for k, v in tg.items()})
    _, sd, _, _ = cases.build(name)
    loss_fn = sel["loss"](cfg, comm_for(c))
    t = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=1e-4)
    t.step(dev)
    osd = t.optimizer_state_dict()
    t2 = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=1e-4)
    t2.load_optimizer_state_dict(osd)
    assert t2.adam_step == 1 and t2.num_it == 0 and all(torch.equal(t2.m[k], t.m[k]) for k in t.m)
    bad = {"state": {i: dict(s) for i, s in osd["state"].items()}, "param_groups": osd["param_groups"]}
    i0 = next(iter(bad["state"]))
    bad["state"][i0]["exp_avg"] = bad["state"][i0]["exp_avg"].reshape(-1)[:-1].clone()
    t3 = trn.FP32Trainer(cfg, comm_for(c), sd_torch(sd), loss_fn, lr=1e-4)
    with pytest.raises(ValueError):
        t3.load_optimizer_state_dict(bad)
    assert not t3.m                                     # nothing was half-loaded
    swapped = {"state": {0: osd["state"][1], 1: osd["state"][0]}, "param_groups": osd["param_groups"]}
    if tuple(osd["state"][0]["exp_avg"].shape) != tuple(osd["state"][1]["exp_avg"].shape):
        with pytest.raises(ValueError):
            t3.load_optimizer_state_dict(swapped)


@pytest.mark.parametrize("conc", ["spat", "temp"])
def test_packed_staging_one_copy_feeds_the_assembler(conc):
    """`PackedStaging`: the per-video items of a batch in ONE pinned host buffer, ONE H2D copy, the assembler reads the device
    views: bit-equal to the reference fixture (as the per-key path), and a refill + second upload replaces every byte."""
    it = mga.items()
    g = np.load(mga.path(conc))
    asm = dls.DeviceBatchAssembler(_asm_cfg(conc), {"num_prop_per_frm": mga.SHAPE["nppf0"]})
    st = dls.PackedStaging({k: np.zeros_like(v) for k, v in it.items()})
    assert st.hbuf.is_pinned() and all(o % 256 == 0 for o, _, _, _ in st.layout.values())
    st.upload()                                      # zeros first: the second upload must replace them
    st.fill(it)
    res = asm(st.upload())
    torch.cuda.synchronize()
    for k in mga.KEYS:
        got = res[k].cpu().numpy()
        assert np.array_equal(got, g[k].astype(got.dtype)), k
    for k, v in it.items():
        assert np.array_equal(st.dev[k].cpu().numpy(), v), k


@pytest.mark.parametrize("hold", [1, 4])
def test_device_prefetcher_hands_out_every_batch_once_and_intact(hold):
    """`DevicePrefetcher`: 40 batches (small arrays packed into one transfer, a large one on its own, a short tail batch of
    another shape in the middle and at the end), copies issued ahead on a copy stream into a ring of persistent buffers. The
    consumer keeps the last `hold` batches it was handed and reads them late (a kernel queue in front): every batch arrives
    once, in order, with its own values, and a buffer set is never rewritten while the consumer may still read it."""
    rng = np.random.default_rng(3)
    def mk(i, b):
        return {"big": torch.from_numpy(rng.standard_normal((b, 40000)).astype(np.float32)).pin_memory(),
                "ids": torch.full((b, 3), i, dtype=torch.int64).pin_memory(),
                "msk": torch.from_numpy(rng.integers(0, 2, (b, 5, 7)).astype(np.uint8)),          # pageable on purpose
                "len": torch.arange(b, dtype=torch.int64) + i}
    batches = [mk(i, 2 if i in (17, 39) else 4) for i in range(40)]
    held, sums = [], []
    busy = torch.randn(2048, 2048, device="cuda")
    n = 0
    for dbt, hbt in dls.DevicePrefetcher(batches, "cuda", depth=2, hold=hold):
        assert hbt is batches[n] and all(v.is_cuda for v in dbt.values()) and list(dbt) == list(hbt)
        held.append((n, dbt))
        held = held[-hold:]
        for _ in range(3):
            busy = busy @ busy * 1e-3                       # the consumer's stream runs behind the host
        for j, d in held:                                   # late reads of everything the consumer may still hold
            sums.append((j, d["big"].double().sum(), d["ids"].sum(), d["msk"].long().sum(), d["len"].sum()))
        n += 1
    assert n == 40
    torch.cuda.synchronize()
    for j, a, b_, c, d in sums:
        h = batches[j]
        assert abs(float(a) - float(h["big"].double().sum())) < 1e-6 * h["big"].numel()
        assert int(b_) == int(h["ids"].sum()) and int(c) == int(h["msk"].long().sum()) and int(d) == int(h["len"].sum()), j


def test_packed_staging_copy_stream_double_buffer():
    """`upload_on` (copy stream, two device buffers): three batches in a row, each assembled from the buffer its copy landed
    in, while the next copy is already issued - every result equals the assembly of ITS items (no copy overtakes a reader)."""
    conc = "spat"
    it = mga.items()
    asm = dls.DeviceBatchAssembler(_asm_cfg(conc), {"num_prop_per_frm": mga.SHAPE["nppf0"]})
    st = dls.PackedStaging({k: np.zeros_like(v) for k, v in it.items()}, n_dev=2)
    cs = torch.cuda.Stream()
    outs, refs = [], []
    for i in range(3):
        cur = {k: (v + (i if v.dtype.kind == "f" else 0)).astype(v.dtype) for k, v in it.items()}
        torch.cuda.current_stream().synchronize() if i == 0 else None
        cs.synchronize()                                  # the host buffer is free again (its previous copy has left it)
        st.fill(cur)
        d = st.upload_on(cs)
        res = asm(d, with_loss_keys=False)
        st.release()
        outs.append({k: res[k].clone() for k in dls.FWD_KEYS})
        ref = asm({k: torch.from_numpy(v).cuda() for k, v in cur.items()}, with_loss_keys=False)
        refs.append({k: ref[k].clone() for k in dls.FWD_KEYS})
    torch.cuda.synchronize()
    for o, r in zip(outs, refs):
        for k in dls.FWD_KEYS:
            assert torch.equal(o[k], r[k]), k


# ---- round 5: a stalled BiLSTM hand-off is an error at the API, never NaN scores with rc 0 -----------------------------
def test_stalled_handoff_raises_on_the_eager_path_and_degrades():
    """`lstm_inject_stall`: every persistent layer launch behaves as if its hand-off had timed out (outputs poisoned with NaN,
    the sticky counter in pinned host memory bumped). The NEXT host-visible point raises VogError; the engine has switched to
    the step-launch BiLSTM, which cannot stall: the re-run of the batch is finite and matches the reference golden."""
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    eng = mdl.engine()
    ok = mdl(dev)
    torch.cuda.synchronize()
    mdl.check_faults()                                        # nothing stalled
    eng.set_option("lstm_inject_stall", 1)
    bad = mdl(dev)
    torch.cuda.synchronize()
    assert not torch.isfinite(bad["mdl_outs_eval"]).all()     # the poison reaches the scores ...
    with pytest.raises(L.VogError, match="hand-off"):
        mdl.check_faults()                                    # ... and the API says so
    assert eng.stalls >= 1                                    # (counted per layer launch: 2 per forward)
    again = mdl(dev)                                          # degraded: step launches (the hook only touches the layer kernel)
    torch.cuda.synchronize()
    mdl.check_faults()
    assert torch.isfinite(again["mdl_outs_eval"]).all()
    g = np.load(cases.golden_path(name))
    pred = eng.unpack_pred(again["_pred_rec"], batch["new_srl_idxs"].shape[1])
    _check_against(name, again, pred, g, None, tol_rel=1e-3, tol_logit=6e-3)
    # a forward() issued after an unnoticed stall raises before it enqueues anything
    eng.set_option("lstm_persistent", 1)
    mdl(dev)
    torch.cuda.synchronize()
    with pytest.raises(L.VogError, match="hand-off"):
        mdl(dev)


def test_stalled_handoff_raises_from_a_graph_slot():
    name = "full/cfg2_ragged"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    eng = mdl.engine()
    eng.set_option("lstm_inject_stall", 1)
    slot = eng.make_slot({k: v for k, v in dev.items() if k in batch}, graph=True)
    eng.set_option("lstm_inject_stall", 0)                    # (captured into the slot's graph)
    slot.launch()
    torch.cuda.synchronize()
    assert not torch.isfinite(slot.out["mdl_outs_eval"]).all()
    with pytest.raises(L.VogError, match="hand-off"):
        slot.launch()                                          # the next use of the slot
    # a fresh slot captured now runs the step-launch BiLSTM
    s2 = eng.make_slot({k: v for k, v in dev.items() if k in batch}, graph=True)
    s2.launch()
    torch.cuda.synchronize()
    s2.check()
    assert torch.isfinite(s2.out["mdl_outs_eval"]).all()


def test_stall_confined_to_one_direction_is_still_an_error():
    """the hand-off slots and the residency wait are per direction. `lstm_inject_stall = 2` makes only the workgroups
    of direction 1 end dead - direction 0, workgroup (0, 0) included, finishes clean, as it does when a late workgroup of
    direction 1 is the only one left without a CU. The sticky counter still has to move (whichever workgroup ends dead first
    reports), once per layer launch, and the scores are poisoned through direction 1's half of the layer output."""
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    eng = mdl.engine()
    eng.set_option("lstm_inject_stall", 2)
    slot = eng.make_slot({k: v for k, v in dev.items() if k in batch}, graph=True)
    eng.set_option("lstm_inject_stall", 0)
    slot.launch()
    torch.cuda.synchronize()
    assert not torch.isfinite(slot.out["mdl_outs_eval"]).all()
    assert int(slot._fault[0]) == 2                            # one report per layer launch, not one per dead workgroup
    with pytest.raises(L.VogError, match="hand-off"):
        slot.check()
    eng.set_option("lstm_persistent", 1)                       # (the engine degraded; back for the second launch's count)
    slot._fault_seen = int(slot._fault[0])
    slot.launch()
    torch.cuda.synchronize()
    assert int(slot._fault[0]) == 4                            # sync[3] is re-armed by every forward's prologue


def test_evaluator_refuses_to_write_a_pickle_with_poisoned_scores(tmp_path):
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    loss_fn = sel["loss"](cfg, comm_for(c))
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    cpu = {k: v.cpu() for k, v in dev.items()}
    cpu.update({k: torch.from_numpy(v) for k, v in tg.items()})
    mdl.engine().set_option("lstm_inject_stall", 1)
    with pytest.raises(L.VogError, match="hand-off"):
        evl(mdl, loss_fn, _Loader([cpu, cpu, cpu]), "valid", rank=0, pred_path=tmp_path)
    assert not (tmp_path / "valid_0.pkl").exists()
    # the engine has degraded: the same call now completes with finite records
    val_loss, _ = evl(mdl, loss_fn, _Loader([cpu, cpu, cpu]), "valid", rank=0, pred_path=tmp_path)
    recs = pickle.load(open(tmp_path / "valid_0.pkl", "rb"))
    assert len(recs) == 3 * batch["num_cmp_msk"].shape[0] and np.isfinite(float(val_loss["loss"]))
    assert all(np.isfinite(np.array(r["pred_scores"])).all() for r in recs)


def test_oversubscribed_persistent_layers_never_pass_nan_silently():
    """Eight graph slots launched on eight streams AROUND the lane book (raw vog_graph_launch): up to 8 persistent layer kernels
    compete for the CUs 4 of them fill. Whether hand-offs stall depends on how the hardware deals the workgroups; what must
    hold is the contract: non-finite outputs <=> the slot's stall counter moved (and `check` raises)."""
    import ctypes as C
    name = "full/cfg2_vog_spat_gt5_bs4"
    cfg, sel, mdl, evl, dev, batch, c = _build(name)
    eng = mdl.engine()
    inp = {k: v for k, v in dev.items() if k in batch}
    slots = [eng.make_slot(inp, graph=True) for _ in range(8)]
    streams = [torch.cuda.Stream() for _ in range(8)]
    torch.cuda.synchronize()
    for it in range(20):
        for sl, st in zip(slots, streams):
            L.check(eng.lib.vog_graph_launch(sl.graph, st.cuda_stream), "vog_graph_launch")
    torch.cuda.synchronize()
    stalled = 0
    for sl in slots:
        finite = bool(torch.isfinite(sl.out["mdl_outs_eval"]).all())
        moved = int(sl._fault[0]) != sl._fault_seen
        stalled += int(moved)
        assert finite or moved, "NaN outputs without a recorded stall"
        if moved:
            with pytest.raises(L.VogError):
                sl.check()
        else:
            sl.check()
    print(f"oversubscription: {stalled} of 8 slots recorded a stall in 20 rounds")
