"""Autograd through the model and the loss (autograd.py): `loss_fn(mdl(b), b)['loss'].backward()` fills `p.grad`
on the device fp32 path - against the reference's autograd (tests/golden/bwd__*.npz), against the closed loop
(`FP32Trainer.gradients` / `.step`), against autograd through the CPU oracle for what the closed loop never needed
(mdl_outs_eval, the sep verb head, input features), with frozen parameters, train-mode dropout and
DistributedDataParallel; and the no-grad path left as it was."""
import importlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cases
from oracle import make_golden_bwd as mgb
from oracle import vog_oracle as vo
from tests.gpu_util import comm_for
from tests.test_bwd_oracle import check_fixture

pytestmark = pytest.mark.gpu

synth = importlib.import_module("vognet-pytorch_amd.synth")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
trn = importlib.import_module("vognet-pytorch_amd.train")
BW = importlib.import_module("vognet-pytorch_amd.backward")
AG = importlib.import_module("vognet-pytorch_amd.autograd")
L = importlib.import_module("vognet-pytorch_amd.lib")

LANG = ("lstm_encoder.", "lstm_out_feat_proj.", "srl_arg_words_out_enc.")


def _build(name):
    cfg, sd, batch, c = cases.build(name)
    sel = sel_mod.get_mdl_loss_eval(cfg)
    comm = comm_for(c)
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    loss_fn = sel["loss"](cfg, comm)
    return cfg, sd, batch, tg, c, mdl.cuda(), dev, loss_fn


def _grads(mdl):
    return {n: p.grad.detach().clone() for n, p in mdl.named_parameters() if p.grad is not None}


def _oracle(cfg, sd, batch, tg, c, drop=None, feat_grad=False):
    """autograd through the CPU oracle -> (forward out, loss dict, parameters, inputs)."""
    oc = vo.OracleCfg.from_cfg(cfg, c["vocab"], c["nppf0"])
    sdt = {k: v.clone().requires_grad_(True) for k, v in vo.to_torch(sd).items()}
    inp = vo.to_torch({**batch, **tg})
    if feat_grad:
        inp["pad_region_feature"] = inp["pad_region_feature"].clone().requires_grad_(True)
    torch.set_num_threads(8)
    kw = {}
    if drop is not None:
        kw = dict(drop=drop, p_obj=float(cfg.mdl.obj_tx.attn_drop), p_mul=float(cfg.mdl.mul_tx.attn_drop))
    out = vo.forward(oc, sdt, inp, **kw)
    ld = vo.loss_forward(oc, out, inp, loss_lambda=float(cfg.loss.loss_lambda))
    return out, ld, sdt, inp


def _close(got, ref, tol, what=""):
    scale = max(float(ref.abs().max()), 1e-12)
    err = float((got.detach().cpu() - ref).abs().max())
    assert err <= tol * scale, (what, err, scale)
    return err / scale


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "small/vog_sep_cmpmsk", "small/igrnd_spat",
                                  "small/vgrnd_temp", "full/cfg2_vog_spat_gt5_bs4", "full/cfg5_vog_svsq_gt5_bs16"])
def test_loss_backward_vs_reference_autograd(name):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval().requires_grad_(True)
    ld = loss_fn(mdl(dev), dev)
    assert ld["loss"].grad_fn is not None
    ld["loss"].backward()
    g = np.load(mgb.bwd_path(name))
    assert abs(float(ld["loss"].detach()) - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    have = {k[2:-len("__shape")] for k in g.files if k.startswith("p:") and k.endswith("__shape")}
    grads = _grads(mdl)
    assert set(grads) == have, (set(grads) ^ have)
    worst = max(check_fixture(g, "p:" + k, v.cpu().numpy(), tol=5e-3) for k, v in grads.items())
    print(name, "worst relative gradient error", worst)


@pytest.mark.parametrize("name", ["small/vog_spat", "full/cfg2_vog_spat_gt5_bs4", "full/cfg5_vog_svsq_gt5_bs16"])
def test_autograd_equals_closed_loop(name):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    tr = trn.FP32Trainer(cfg, comm_for(c), {k: torch.from_numpy(v) for k, v in sd.items()}, loss_fn, lr=1e-4)
    _, ref = tr.gradients(dev)
    mdl.eval().requires_grad_(True)
    loss_fn(mdl(dev), dev)["loss"].backward()
    got = _grads(mdl)
    assert set(got) == set(ref)
    for k, v in ref.items():
        _close(got[k], v.cpu(), 1e-6, k)
    # three optimizer steps against three FP32Trainer steps
    mdl.zero_grad(set_to_none=True)
    opt = torch.optim.Adam(mdl.parameters(), lr=1e-4, betas=(0.9, 0.99))
    for _ in range(3):
        opt.zero_grad()
        l_ag = loss_fn(mdl(dev), dev)["loss"]
        l_ag.backward()
        opt.step()
        l_tr = tr.step(dev)["loss"]
        assert abs(float(l_ag.detach()) - float(l_tr)) <= 1e-6 * abs(float(l_tr))
    # parameters: torch.optim.Adam and vog_adam_f32 round differently, and Adam's normalisation lifts last-bit differences of
    # near-zero gradients (dead ReLU rows of prop_encoder, unused embedding columns) to a visible fraction of a step (measured
    # at cfg 2: 1.4 % of lr on one entry of weight_ih_l0, 3.8e-6 relative in norm on prop_encoder.0.weight) - the losses above
    # agree to 1e-6; here: 1e-6 relative in norm over all parameters, hardly any entry off by more than 5 % of a step, none
    # by more than one step
    after = tr.state_dict()
    lr, bad, tot, dn, rn = 1e-4, 0, 0, 0.0, 0.0
    for n, p in mdl.named_parameters():
        ref = after[n].cpu().double()
        diff = (p.detach().cpu().double() - ref).abs()
        assert float(diff.max()) <= lr, n
        bad += int((diff > 0.05 * lr).sum())
        tot += diff.numel()
        dn += float((diff ** 2).sum())
        rn += float((ref ** 2).sum())
    assert dn ** 0.5 <= 1e-6 * rn ** 0.5 and bad <= 1e-3 * tot, (dn ** 0.5 / rn ** 0.5, bad, tot)


@pytest.mark.parametrize("name", ["small/vog_sep_cmpmsk", "full/cfg5_vog_svsq_gt5_bs16"])
def test_verb_loss_backward_vs_oracle(name):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval().requires_grad_(True)
    ld = loss_fn(mdl(dev), dev)
    (ld["loss"] + ld["verb_loss"]).backward()
    _, ol, sdt, _ = _oracle(cfg, sd, batch, tg, c)
    (ol["loss"] + ol["verb_loss"]).backward()
    got = _grads(mdl)
    assert {k for k, v in sdt.items() if v.grad is not None} == set(got)
    for k in got:
        _close(got[k], sdt[k].grad, 5e-3, k)
    # the verb head's contribution reaches seg_verb_classf, the segment encoder and the LSTM
    mdl.zero_grad(set_to_none=True)
    loss_fn(mdl(dev), dev)["loss"].backward()
    no_verb = _grads(mdl)
    assert "seg_verb_classf.0.weight" in got and "seg_verb_classf.0.weight" not in no_verb
    for k in ("seg_encoder.0.weight", "lstm_encoder.lstm.weight_hh_l0", "lstm_out_feat_proj.0.weight"):
        assert not torch.equal(got[k], no_verb[k]), k


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_temp", "small/vog_sep_cmpmsk"])
def test_mdl_outs_eval_backward_vs_oracle(name):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval().requires_grad_(True)
    out = mdl(dev)
    R = torch.randn(out["mdl_outs_eval"].shape, generator=torch.Generator().manual_seed(5))
    (out["mdl_outs_eval"] * R.cuda()).sum().backward()
    oout, _, sdt, _ = _oracle(cfg, sd, batch, tg, c)
    (oout["mdl_outs_eval"] * R).sum().backward()
    got = _grads(mdl)
    for k in got:
        _close(got[k], sdt[k].grad, 5e-3, k)
    # masked positions contribute exactly 0: the gradient reaching the logits through the masks alone
    lg = out["mdl_outs"].detach().contiguous()
    d_logits = torch.empty_like(lg)
    B, nc_v, nsrl, NP = lg.shape
    d = mdl._grad_trainer.desc
    am, cm = dev["srl_arg_inds_msk"].contiguous(), dev["num_cmp_msk"].contiguous()
    Rd = R.cuda().contiguous()
    L.check(L.load().vog_score_eval_bwd_f32(L.ptr(lg), None, L.ptr(Rd), L.ptr(am), L.ptr(cm),
                                            L.ptr(d_logits), B * nc_v, nsrl, NP, d.conc_type, cm.shape[1], nc_v, am.shape[1], d.nfrm0,
                                            d.nppf0, L.stream_ptr()), "vog_score_eval_bwd_f32")
    masked = (out["mdl_outs_eval"].detach() == 0)
    assert masked.any()
    assert (d_logits[masked] == 0).all()


def _frozen_run(name, trainable):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval()
    for n, p in mdl.named_parameters():
        p.requires_grad_(trainable(n))
    loss_fn(mdl(dev), dev)["loss"].backward()
    return _grads(mdl), mdl


def test_freezing_language_side(monkeypatch):
    name = "small/vog_spat"
    full, _ = _frozen_run(name, lambda n: True)
    orig = BW.language_backward

    def forward_only(*a, **k):                                    # (the forward runs the language side through it too)
        if k.get("d_lang_enc") is not None:
            raise AssertionError("language_backward called with the language side frozen")
        return orig(*a, **k)

    monkeypatch.setattr(BW, "language_backward", forward_only)
    fr, mdl = _frozen_run(name, lambda n: not n.startswith(LANG))
    for n, p in mdl.named_parameters():
        if n.startswith(LANG):
            assert p.grad is None, n
    assert set(fr) == {k for k in full if not k.startswith(LANG)}
    for k in fr:
        assert torch.equal(fr[k], full[k]), k


def test_freezing_all_but_lin2_and_mul_tx():
    name = "small/vog_spat"
    full, _ = _frozen_run(name, lambda n: True)
    fr, _ = _frozen_run(name, lambda n: n.startswith(("lin2.", "mult_txf.")))
    assert set(fr) == {k for k in full if k.startswith(("lin2.", "mult_txf."))}
    for k in fr:
        assert torch.equal(fr[k], full[k]), k


@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep_r64"])
def test_dropout_masks_match_oracle(name):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.train().requires_grad_(True)
    seed = AG.next_dropout_seed(mdl)
    ld = loss_fn(mdl(dev), dev)
    ld["loss"].backward()
    _, ol, sdt, _ = _oracle(cfg, sd, batch, tg, c, drop=seed)
    ol["loss"].backward()
    assert abs(float(ld["loss"].detach()) - float(ol["loss"])) <= 2e-5 * abs(float(ol["loss"]))
    got = _grads(mdl)
    for k in got:
        _close(got[k], sdt[k].grad, 5e-3, k)
    # the next call draws other masks
    assert AG.next_dropout_seed(mdl) != seed
    o1 = mdl(dev)["mdl_outs"].detach().clone()
    o2 = mdl(dev)["mdl_outs"].detach().clone()
    assert not torch.equal(o1, o2)


def test_default_path_unchanged_and_optimizer_updates_reach_the_engine():
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval()
    out = mdl(dev)                                              # no parameter requires grad
    ref = mdl.engine().forward(dev)
    for k in ("mdl_outs", "mdl_outs_eval"):
        assert out[k].grad_fn is None and torch.equal(out[k], ref[k]), k
    mdl.requires_grad_(True)
    with torch.no_grad():
        out = mdl(dev)
    for k in ("mdl_outs", "mdl_outs_eval"):
        assert out[k].grad_fn is None and torch.equal(out[k], ref[k]), k
    opt = torch.optim.Adam(mdl.parameters(), lr=1e-3, betas=(0.9, 0.99))
    loss_fn(mdl(dev), dev)["loss"].backward()
    opt.step()
    with torch.no_grad():
        got = mdl(dev)
    fresh = sel_mod.get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm_for(c))
    fresh.load_state_dict({k: v.detach().cpu() for k, v in mdl.state_dict().items()})
    fresh = fresh.cuda().eval()
    with torch.no_grad():
        exp = fresh(dev)
    assert not torch.equal(got["mdl_outs"], ref["mdl_outs"])
    for k in ("mdl_outs", "mdl_outs_eval"):
        assert torch.equal(got[k], exp[k]), k


def test_input_feature_gradient_and_errors():
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval()
    dev["pad_region_feature"] = dev["pad_region_feature"].clone().requires_grad_(True)
    loss_fn(mdl(dev), dev)["loss"].backward()
    _, ol, sdt, inp = _oracle(cfg, sd, batch, tg, c, feat_grad=True)
    ol["loss"].backward()
    _close(dev["pad_region_feature"].grad, inp["pad_region_feature"].grad, 5e-3, "pad_region_feature")
    assert all(p.grad is None for p in mdl.parameters())
    dev["pad_region_feature"] = dev["pad_region_feature"].detach()
    bad = dict(dev)
    bad["pad_proposals"] = bad["pad_proposals"].clone().requires_grad_(True)
    with pytest.raises(L.VogError, match="pad_proposals"):
        mdl(bad)
    mdl.requires_grad_(True)
    w = getattr(mdl.lin2, "0").weight
    w.data = w.data.cpu()
    with pytest.raises(L.VogError, match="lin2.0.weight"):
        mdl(dev)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_batch(cfg, c, rank):
    b = synth.make_batch(cfg.ds.conc_type, 2, c["nppf0"], ncmp=c["ncmp"], vocab_size=c["vocab"], prop_dim=cfg.mdl.prop_feat_dim,
                         seg_dim=cfg.mdl.seg_feat_dim, seed=4300 + rank, ragged=True)
    b.update(synth.make_targets(b, cfg.ds.conc_type, c["nppf0"], seed=91 + rank))
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}


def _ddp_worker(rank, world, port, name, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval().requires_grad_(True)
    ddp = torch.nn.parallel.DistributedDataParallel(mdl, find_unused_parameters=True)
    b = _rank_batch(cfg, c, rank)
    loss = loss_fn(ddp(b), b)["loss"].mean()
    loss.backward()
    torch.cuda.synchronize()
    q.put((rank, {n: p.grad.cpu().numpy() for n, p in mdl.named_parameters() if p.grad is not None}))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_two_ranks_average_the_gradients():
    name, world = "small/vog_spat", 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_ddp_worker, args=(r, world, port, name, q)) for r in range(world)]
    for p in ps:
        p.start()
    got = {}
    for _ in range(world):
        r, g = q.get(timeout=300)
        got[r] = g
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    mdl.eval().requires_grad_(True)
    single = []
    for r in range(world):
        mdl.zero_grad(set_to_none=True)
        b = _rank_batch(cfg, c, r)
        loss_fn(mdl(b), b)["loss"].backward()
        single.append(_grads(mdl))
    for r in range(world):                                        # (parameters no rank used: None, or zeros from the reducer)
        assert set(single[0]) <= set(got[r])
        assert all(not got[r][k].any() for k in set(got[r]) - set(single[0]))
    for k in single[0]:
        mean = (single[0][k] + single[1][k]).cpu() / 2
        for r in range(world):
            _close(torch.from_numpy(got[r][k]), mean, 1e-6, k)
