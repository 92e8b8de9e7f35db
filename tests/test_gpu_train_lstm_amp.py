"""The K-split mixed-precision BiLSTM recurrence of the training path (`vog_train_set_int("lstm_amp_split", 1)` under "amp":
lstm_ksplit_{fwd,bwd}_kernel<Op16> in csrc/train_lang.hip) on the device: `vog_lang_f32` against the rounded torch restatement of
tests/test_gpu_amp.py, against the tile kernels under the same bounds, the switch's isolation from the fp32 path, scratch guard
bands, reproducibility, frozen weights, the launch counter, and the switch through the trainer, the autograd path and the
Learner. Every test sets the switch in a try / finally that resets it."""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import tests.test_gpu_amp as amp_tests
from tests.test_gpu_amp import MODES, _check, _compare, _sd
from tests.test_gpu_train_ops import LANG_4, LANG_OVER, _lang_case, _lang_dev, _lang_nb, _ShortBy1, guarded, language_call

pytestmark = pytest.mark.gpu
bwd = importlib.import_module("vognet-pytorch_amd.backward")
L = bwd.L
ACTS = ("_lang_enc", "_full", "_hid")
LANG_24 = (24, [1, 7, 3, 5, 2, 6, 4, 7, 1, 3, 5, 2, 6, 4, 7, 1, 2, 3, 4, 5, 6, 7, 1, 2], 8, 16, 2, 6, 5)   # two sentence tiles, the second partial


def _get(name):
    v = C.c_int(-7)
    assert L.load().vog_train_get_int(name, C.byref(v)) == 0
    return v.value


@contextlib.contextmanager
def amp_split(on=1, amp=1):
    """The calling thread's switches for the calls inside, reset behind them; the launch counter starts at 0."""
    lib = L.load()
    try:
        assert lib.vog_train_set_int(b"lstm_amp_split", on) == 0
        assert lib.vog_train_set_int(b"amp", amp) == 0
        assert lib.vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
        yield
    finally:
        lib.vog_train_set_int(b"lstm_amp_split", 0)
        lib.vog_train_set_int(b"amp", 0)


def _run(c, on, amp=1, **kw):
    sd, batch = _lang_dev(c)
    with amp_split(on, amp):
        r = language_call(sd, batch, c["T"], c["dims"][3], d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda(), **kw)
        n = _get(b"lstm_amp_split_launches")
    return sd, r, n


# ---- 1. against the rounded restatement ---------------------------------------------------------------------------------------
def _restatement_T(Bn, R):
    """max(lens) of test_language_amp_vs_rounded_restatement(Bn, R, .): its first draws from its seeded generator."""
    g = torch.Generator().manual_seed(Bn * 77 + R)
    lens = [1] + [int(v) for v in torch.randint(1, 9, (Bn - 1,), generator=g)] if Bn > 1 else [1]
    if Bn > 2:
        lens[2] = 9
    return max(lens)


# The restatement's own spread (float32 against float64 accumulation, on the CPU) stays under the fixed bounds of `_check` in
# every case, so its "twice the spread" clause never widens one: at most 2.4e-3 in the largest entry ((4, 1024, bf16)) against
# 2^-8 = 3.9e-3; (3, 10, bf16): 1.4e-7 in the largest entry, 9.7e-8 in norm.
RESTATED = [(5, 20, "bf16"), (5, 20, "f16"),          # one active wave of four, scalar loads (R % 8 != 0)
            (17, 40, "bf16"),                         # a partial last fragment; two sentence tiles, the second with one row
            (24, 72, "bf16"), (3, 72, "f16"),         # three active waves (chunks of 32, 32, 8)
            (1, 8, "bf16"),                           # one sentence, one step, K below one fragment row
            (3, 10, "bf16"),                          # R not a multiple of 4: the last unit tile partial, no 16-byte load of h
            (4, 1024, "bf16"), (4, 1024, "f16"), (16, 1024, "f16")]      # the model's width: the unrolled vector path


@pytest.mark.parametrize("Bn,R,mode", RESTATED, ids=[f"Bn{b}_R{r}_{m}" for b, r, m in RESTATED])
def test_split_against_the_rounded_restatement(Bn, R, mode):
    """tests/test_gpu_amp.py's yardstick, called as it stands with the switch set around it: its bounds (`_check`), one forward
    call and one backward call from the kept forward - one launch per layer and step each."""
    layers, T = 2, _restatement_T(Bn, R)
    lib = L.load()
    try:
        assert lib.vog_train_set_int(b"lstm_amp_split", 1) == 0
        assert lib.vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
        amp_tests.test_language_amp_vs_rounded_restatement(Bn, R, mode)
        assert _get(b"lstm_amp_split_launches") == 2 * layers * T
    finally:
        lib.vog_train_set_int(b"lstm_amp_split", 0)
    assert _get(b"amp") == 0


# ---- 2. consistency with the tile path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("key", [LANG_4, LANG_OVER], ids=["4_layers", "over_R4"])
def test_split_against_the_tile_path(key, mode):
    """Same operands, same rounding, another order of the fp32 sums: every activation and gradient within `_check`'s bound of the
    tile path's (the tile result is both restatements, so the fixed bounds hold: f16 1e-3 / 1e-3, bf16 2^-8 / 1e-2)."""
    c = _lang_case(*key)
    amp = MODES[mode][1]
    sd, tile, n0 = _run(c, 0, amp)
    sd, split, n1 = _run(c, 1, amp)
    assert n0 == 0 and n1 == 2 * c["dims"][3] * c["T"]
    for k in list(ACTS) + list(sd):
        _check(mode, split[k], tile[k], tile[k], f"split vs tile {k}")


# ---- 3. switch isolation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [LANG_4, LANG_OVER], ids=["4_layers", "over_R4"])
def test_switch_changes_nothing_without_amp(key):
    c = _lang_case(*key)
    sd, off, n0 = _run(c, 0, 0)
    sd, on, n1 = _run(c, 1, 0)
    assert n0 == 0 and n1 == 0
    for k in list(ACTS) + list(sd):
        assert torch.equal(off[k], on[k]), k
    assert _get(b"lstm_amp_split") == 0 and _get(b"amp") == 0


@pytest.mark.parametrize("amp", [1, 2])
def test_counter_stays_zero_under_amp_with_the_switch_off(amp):
    c = _lang_case(*LANG_4)
    _, _, n = _run(c, 0, amp)
    assert n == 0


def test_lstm_fused_keeps_its_contract_under_amp():
    """"lstm_fused" changes nothing under amp, with the new switch set too: the bits are the split path's, its counter stays 0."""
    c = _lang_case(*LANG_OVER)
    sd, a, n = _run(c, 1)
    lib = L.load()
    try:
        assert lib.vog_train_set_int(b"lstm_fused", 1) == 0
        assert lib.vog_train_set_int(b"lstm_fused_launches", 0) == 0
        sd, b, m = _run(c, 1)
        assert _get(b"lstm_fused_launches") == 0
    finally:
        lib.vog_train_set_int(b"lstm_fused", 0)
    assert n == m == 2 * c["dims"][3] * c["T"]
    for k in list(ACTS) + list(sd):
        assert torch.equal(a[k], b[k]), k


# ---- 4. scratch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 252])
def test_misaligned_scratch_base_under_the_switch(shift):
    """Both guard bands intact at either shift (guarded), every output with the bits of the call on an aligned view."""
    c = _lang_case(*LANG_OVER)
    _, base, _ = _run(c, 1)
    sd, got, n = _run(c, 1, shift=shift)
    assert n == 2 * c["dims"][3] * c["T"]
    for k in list(sd) + list(ACTS):
        assert torch.equal(base[k], got[k]), k


def test_scratch_one_byte_short_is_refused_before_any_launch(monkeypatch):
    lib = L.load()
    c = _lang_case(*LANG_OVER)
    sd, batch = _lang_dev(c)
    monkeypatch.setattr(bwd.L, "load", lambda: _ShortBy1(lib, "vog_lang_f32_scratch_bytes"))
    try:
        assert lib.vog_train_set_int(b"amp", 1) == 0
        assert lib.vog_train_set_int(b"lstm_amp_split", 1) == 0
        assert lib.vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
        with pytest.raises(L.VogError, match="rc=-2"):
            bwd.language_backward(sd, batch, c["T"], c["dims"][3], d_lang_enc=c["d_le"].cuda())
        assert _get(b"lstm_amp_split_launches") == 0
    finally:
        lib.vog_train_set_int(b"lstm_amp_split", 0)
        lib.vog_train_set_int(b"amp", 0)


# ---- 5. reproducible; frozen weights; a kept forward of either setting --------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    c = _lang_case(*LANG_24)
    sd, a, _ = _run(c, 1)
    sd, b, _ = _run(c, 1)
    for k in list(sd) + list(ACTS):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("need,bwd_layers", [(("lstm_encoder.lstm.weight_hh_l1_reverse",), 1), (("lstm_encoder.embed_tokens.weight",), 2),
                                             (("srl_arg_words_out_enc.0.bias",), 0)])
def test_need_subsets(need, bwd_layers):
    """Only the wanted gradients come back, with the bits of the call that wants them all, and the backward recurrence ran for
    `bwd_layers` layers only (the chain stops above layer 0 / runs to the embedding / returns behind b_arg)."""
    c = _lang_case(*LANG_OVER)
    sd, every, _ = _run(c, 1)
    sd, r, n = _run(c, 1, need=set(need))
    assert {k for k in r if not k.startswith("_")} == set(need)
    assert n == (c["dims"][3] + bwd_layers) * c["T"]
    for k in list(need) + list(ACTS):
        assert torch.equal(r[k], every[k]), k


@pytest.mark.parametrize("fwd_on", [0, 1])
def test_backward_starts_from_a_kept_forward_of_either_setting(fwd_on):
    """The kept state has one format: a split backward from a tile forward (and from a split one) runs T launches per layer and
    stays within `_check`'s bf16 bound of the split call that recomputes its own forward (bit-equal from a split forward)."""
    c = _lang_case(*LANG_OVER)
    T, layers = c["T"], c["dims"][3]
    sd, whole, _ = _run(c, 1)
    batch = _lang_dev(c)[1]
    with amp_split(fwd_on):
        nb, width = _lang_nb(sd, batch, T, layers)
        with guarded(nb, width) as sc:
            f = bwd.language_backward(sd, batch, T, layers, scratch=sc)
            assert _get(b"lstm_amp_split_launches") == fwd_on * layers * T
            assert L.load().vog_train_set_int(b"lstm_amp_split", 1) == 0
            b = bwd.language_backward(sd, batch, T, layers, forward_scratch=f["_scratch"], d_lang_enc=c["d_le"].cuda(), d_hid=c["d_hid"].cuda())
            assert _get(b"lstm_amp_split_launches") == (fwd_on + 1) * layers * T
    for k in sd:
        if fwd_on:
            assert torch.equal(whole[k], b[k]), k
        else:
            _check("bf16", b[k], whole[k], whole[k], f"split backward from a tile forward {k}")


# ---- 6. through the trainer, the autograd path and the Learner ------------------------------------------------------------------
from tests.gpu_util import comm_for                                         # noqa: E402
from tests.test_gpu_autograd import _build, _close, _grads                  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
NAME = "small/vog_spat"


def test_trainer_refuses_another_string():
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    with pytest.raises(ValueError, match="lstm_amp"):
        trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16", lstm_amp="fused")
    assert trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16").lstm_amp == "tile"


def test_trainer_split_close_to_fp32():
    """tests/test_gpu_amp.py::test_amp_step_close_to_fp32's criteria, for the split recurrence against the fp32 step."""
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    t32 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    t16 = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16", lstm_amp="split")
    l32, g32 = t32.gradients(dev)
    assert L.load().vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
    l16, g16 = t16.gradients(dev)
    assert _get(b"lstm_amp_split_launches") > 0 and _get(b"lstm_amp_split") == 0     # the new kernels ran; the switch is reset behind the call
    assert abs(float(l16["loss"]) - float(l32["loss"])) <= 1e-3 * abs(float(l32["loss"])), (float(l16["loss"]), float(l32["loss"]))
    worst, cos_min, differs = _compare(g32, g16, f"{NAME} bf16 split")
    assert differs and worst <= 0.2 and cos_min >= 0.99, (worst, cos_min)


def test_three_adam_steps_follow_the_default_amp_trainer():
    """Bound: tests/test_gpu_amp.py's for losses over Adam steps (1e-2 of the reference loss)."""
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    ts = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16", lstm_amp="split")
    tt = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16")
    assert L.load().vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
    b = [float(tt.step(dev)["loss"]) for _ in range(3)]
    assert _get(b"lstm_amp_split_launches") == 0                             # the default reaches neither new kernel
    a = [float(ts.step(dev)["loss"]) for _ in range(3)]
    assert _get(b"lstm_amp_split_launches") > 0
    print("    losses split", a, "default", b)
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-2 * abs(y), (a, b)


def test_autograd_path_takes_the_recurrence_from_the_cfg():
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    cfg.hip.train_lstm_amp = "split"
    tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16", lstm_amp="split")
    _, ref = tr.gradients(dev)
    mdl.eval().requires_grad_(True)
    assert L.load().vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ld = loss_fn(mdl(dev), dev)
    ld["loss"].backward()
    assert _get(b"lstm_amp_split_launches") > 0 and _get(b"lstm_amp_split") == 0 and _get(b"amp") == 0
    got = _grads(mdl)
    assert set(got) == set(ref)
    for k, v in ref.items():
        _close(got[k], v.cpu(), 1e-6, k)


def test_learner_trains_split_and_its_checkpoint_loads_into_the_default(tmp_path):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    comm = comm_for(c)
    B, ncmp = batch["num_cmp_msk"].shape
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one, one], valid_dl=[one], test_dl=[one])
    cfg.hip.train_amp = "bf16"
    cfg.hip.train_lstm_amp = "split"
    evl = sel_mod.get_mdl_loss_eval(cfg)["eval"](cfg, comm, torch.device("cuda", 0))
    learn = tu.Learner(uid="S0", data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)
    assert learn.trainer.amp == "bf16" and learn.trainer.lstm_amp == "split"
    assert L.load().vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
    hist = learn.fit(epochs=1, lr=1e-4)
    assert len(hist) == 1 and np.isfinite(hist[0]["trn_loss"]) and learn.num_it == 2
    assert _get(b"lstm_amp_split_launches") > 0 and _get(b"lstm_amp_split") == 0 and _get(b"amp") == 0
    learn.save_model_dict()
    cfg2, sd2, _, _, _, mdl2, _, loss2 = _build(NAME)
    assert cfg2.hip.train_lstm_amp == "tile" and cfg2.hip.train_amp == ""
    learn2 = tu.Learner(uid="S0", data=data, mdl=mdl2, loss_fn=loss2, cfg=cfg2,
                        eval_fn=sel_mod.get_mdl_loss_eval(cfg2)["eval"](cfg2, comm, torch.device("cuda", 0)), comm=comm)
    assert learn2.trainer.lstm_amp == "tile" and learn2.trainer.amp is None
    for k, v in learn.trainer.state_dict().items():
        assert torch.equal(v, learn2.trainer.params[k]), k
    assert learn2.trainer.num_it == 2
