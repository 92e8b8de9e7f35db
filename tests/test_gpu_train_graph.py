"""The captured training step (`FP32Trainer.capture` -> `TrainSlot`): one graph launch per iteration, every per-step value in
device memory. Operator level: the step block's tick kernel, the device-counted optimiser against the host-counted entries (bit
for bit), the pinned split-K buffer. Trainer level: four replays on two alternating batches against four eager steps with the
same sentence bound T - parameters, moments and per-step losses `torch.equal` in every mode the step has -, the slot's
staleness and resynchronisation rules, and `Learner.train_epoch` with cfg.hip.train_graph."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests.gpu_util import comm_for
from tests.test_gpu_autograd import _build
from tests.test_gpu_opt import B1, B2, EPS, LR, NAME, SIZES, _dev, _host, _opt_step, _same, _sd
from tests.test_gpu_opt_variants import _ex_step, _fill, _garr

pytestmark = pytest.mark.gpu

trn = importlib.import_module("vognet-pytorch_amd.train")
L = importlib.import_module("vognet-pytorch_amd.lib")
BW = importlib.import_module("vognet-pytorch_amd.backward")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
SEP = "small/vog_sep_cmpmsk"


# ---------------------------------------------------------------- operator level
def _block(tick=0, adam_step=0, clamped=0):
    h = L.TrainStep(tick=tick, adam_step=adam_step, len_clamped=clamped)
    return torch.frombuffer(bytearray(bytes(h)), dtype=torch.int32).cuda()


def _read_block(b):
    return L.TrainStep.from_buffer_copy(b.cpu().numpy().tobytes())


def _tick(block, phase, lens=None, T=0, src=None, ring=None, rows=0, n_loss=0, count_adam=0, cap=None):
    L.check(L.load().vog_train_tick(L.ptr(block), L.ptr(lens), 0 if lens is None else lens.numel(), T, L.ptr(src), L.ptr(ring), rows,
                                    n_loss, phase, count_adam, L.ptr(cap), 0 if cap is None else cap.numel(), L.stream_ptr()),
            "vog_train_tick")
    torch.cuda.synchronize()


def test_tick_clamps_lengths_logs_its_row_and_counts():
    blk = _block(tick=5, adam_step=2)
    lens = torch.tensor([1, 5, 3, 2, 5, 4, 1], dtype=torch.int64, device="cuda")
    _tick(blk, L.TICK_BEGIN, lens, T=5)
    s = _read_block(blk)
    assert lens.tolist() == [1, 5, 3, 2, 5, 4, 1] and (s.tick, s.adam_step, s.len_clamped) == (5, 2, 0)      # none exceeded
    cap = torch.tensor([[0, 4], [3, 3], [2, 1]], dtype=torch.int64, device="cuda")
    _tick(blk, L.TICK_BEGIN, lens, T=5, cap=cap)
    assert cap.tolist() == [[0, 4], [3, 3], [2, 1]] and _read_block(blk).len_clamped == 0
    cap2 = torch.tensor([[0, 5], [-1, 3], [2 ** 35, 1]], dtype=torch.int64, device="cuda")
    b2 = _block()
    _tick(b2, L.TICK_BEGIN, lens, T=5, cap=cap2)
    assert cap2.tolist() == [[0, 4], [0, 3], [4, 1]] and lens.tolist() == [1, 5, 3, 2, 5, 4, 1] and _read_block(b2).len_clamped == 1
    lens = torch.tensor([1, 9, 3, 6, 5, 4, 2 ** 40], dtype=torch.int64, device="cuda")
    _tick(blk, L.TICK_BEGIN, lens, T=5)
    s = _read_block(blk)
    assert lens.tolist() == [1, 5, 3, 5, 5, 4, 5] and (s.tick, s.adam_step, s.len_clamped) == (5, 2, 1)
    _tick(blk, L.TICK_BEGIN, torch.ones(7, dtype=torch.int64, device="cuda"), T=5)
    assert _read_block(blk).len_clamped == 1                                                               # sticky
    # the loss log: row tick % 3 and its marker, tick + 1; the ring wraps
    ring = torch.zeros(3, 3, dtype=torch.float32, device="cuda")
    want = torch.zeros(3, 3, dtype=torch.float32)
    for k in range(5):
        src = torch.tensor([0.25 + k, -1.5 * k, 99.0], dtype=torch.float32, device="cuda")                 # (n_loss = 2: 99 is not copied)
        _tick(blk, L.TICK_END, src=src, ring=ring, rows=3, n_loss=2, count_adam=k % 2)
        tick = 5 + k
        want[tick % 3, :2] = src[:2].cpu()
        want.view(torch.int32)[tick % 3, 2] = tick + 1
        s = _read_block(blk)
        assert (s.tick, s.adam_step, s.len_clamped) == (tick + 1, 2 + (k + 1) // 2, 1)
        assert torch.equal(ring.cpu().view(torch.int32), want.view(torch.int32)), k
    _tick(blk, L.TICK_END)                                                                                  # no ring: the counts only
    assert _read_block(blk).tick == 11 and torch.equal(ring.cpu().view(torch.int32), want.view(torch.int32))


def _bias_table(b1=B1, b2=B2):
    lib, n = L.load(), C.c_int(0)
    assert lib.vog_opt_bias_table(b1, b2, None, 0, C.byref(n)) == -2
    host = (C.c_float * (2 * n.value))()
    L.check(lib.vog_opt_bias_table(b1, b2, host, n.value, C.byref(n)), "vog_opt_bias_table")
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.float32).cuda(), n.value


def _dev_step(p, g, m, v, lrs, groups, block=None, bias=None, vmax=None, flags=0, state=None, max_norm=0.0, growth=(2.0, 0.5, 2000)):
    """vog_opt_step_dev_f32: the group rates from a device table (the groups' own lr fields hold a poison value)."""
    ex = L.OptExArgs()
    keep = _fill(ex.groups.base, p, g, m, v, state, 0, max_norm, growth)
    garr = _garr([(f, c, 123.0, wd) for f, c, _, wd in groups])
    ex.groups.groups, ex.groups.n_groups = garr, len(groups)
    ex.flags, ex.grad_scale = flags, 1.0
    if vmax is not None:
        vm = (C.c_void_p * len(p))()
        for i in range(len(p)):
            vm[i] = L.ptr(vmax[i])
        ex.vmax = vm
    table = torch.tensor(lrs, dtype=torch.float32, device="cuda")
    d = L.OptDevArgs()
    d.lr = L.ptr(table)
    if block is not None:
        d.step, d.bias, d.bias_len = L.ptr(block), L.ptr(bias[0]), bias[1]
    L.check(L.load().vog_opt_step_dev_f32(C.byref(ex), C.byref(d), L.stream_ptr()), "vog_opt_step_dev_f32")
    torch.cuda.synchronize()


def test_device_counted_step_equals_mode_a_at_every_update_number():
    h = _host()
    bias = _bias_table()
    n_tab = bias[1]
    assert abs(n_tab - 1725) <= 2
    g = _dev(h["gs"][2], 1)
    for number in (1, 2, 100, n_tab - 1, n_tab, n_tab + 1, 5000):
        a = [_dev(h["p"], 0), _dev(h["m"], 2), _dev(h["v"], 3)]
        b = [_dev(h["p"], 0), _dev(h["m"], 2), _dev(h["v"], 3)]
        _opt_step(a[0], g, a[1], a[2], step=number)
        blk = _block(tick=7, adam_step=number - 1)
        _dev_step(b[0], g, b[1], b[2], [LR], [(0, len(SIZES), LR, 0.0)], block=blk, bias=bias)
        for k in range(3):
            assert _same(a[k], b[k]), (number, "pmv"[k])
        s = _read_block(blk)
        assert (s.tick, s.adam_step) == (7, number - 1)                  # the optimiser reads the block; the tick's end counts
        assert not all(torch.equal(x.cpu(), y) for x, y in zip(a[0], h["p"]))


@pytest.mark.parametrize("mode_b", [False, True])
def test_device_lr_table_with_two_groups_adamw_amsgrad_equals_the_extended_step(mode_b):
    h = _host()
    n = len(SIZES)
    flags = L.OPT_DECOUPLED | L.OPT_AMSGRAD
    bias = _bias_table()
    mk = lambda: [_dev(h["p"], 0), _dev(h["m"], 2), _dev(h["v"], 3), _dev(h["v"], 3)]
    a, b = mk(), mk()
    sa = sb = None
    if mode_b:
        from tests.test_gpu_opt import _read, _state
        sa, sb = _state(scale=4.0, adam_step=2), _state(scale=4.0, adam_step=2)
    blk = _block(adam_step=2)
    for k, lrs in enumerate([(1e-3, 3e-4), (1e-3, 3e-4), (2.5e-4, 7e-3)]):            # the table changes before the third update
        lrs = [float(np.float32(x)) for x in lrs]
        groups = [(0, 40, lrs[0], 0.01), (40, n - 40, lrs[1], 0.1)]
        g = _dev(h["gs"][k], 1)
        _ex_step(a[0], g, a[1], a[2], vmax=a[3], groups=groups, flags=flags, state=sa, step=3 + k, max_norm=1.0)
        _dev_step(b[0], g, b[1], b[2], lrs, groups, block=None if mode_b else blk, bias=bias, vmax=b[3], flags=flags, state=sb,
                  max_norm=1.0)
        if not mode_b:
            L.check(L.load().vog_train_tick(L.ptr(blk), None, 0, 0, None, None, 0, 0, L.TICK_END, 1, None, 0, L.stream_ptr()), "vog_train_tick")
        for j in range(4):
            assert _same(a[j], b[j]), (k, "pmvx"[j])
    if mode_b:
        assert torch.equal(sa.cpu(), sb.cpu()) and _read(sb).adam_step == 5
    else:
        assert _read_block(blk).adam_step == 5


def _scratch_info(stream):
    p, n, pin = C.c_void_p(0), C.c_size_t(0), C.c_int(0)
    L.check(L.load().vog_train_scratch_info(stream.cuda_stream, C.byref(p), C.byref(n), C.byref(pin)), "vog_train_scratch_info")
    return p.value, n.value, pin.value


def test_pinned_splitk_buffer_refuses_to_grow():
    """A weight gradient over 2048 rows takes the split-K path (8 slices of [128, 256] partials). On a stream whose buffer is
    pinned while it holds less than that - here: nothing - the product is refused with a message and the buffer stays where
    (and what) it was; unpinned it allocates, and pinned again the same product runs in place. (A pinned buffer that has
    been allocated cannot be outgrown: the split-K rule bounds the partials at 8 MiB, the buffer starts at 16.)"""
    lib = L.load()
    streams = [torch.cuda.Stream() for _ in range(40)]                  # torch hands out pooled handles: take one no product ran on
    fresh = [t for t in streams if _scratch_info(t)[1] == 0 and _scratch_info(t)[2] == 0]
    assert fresh, "every pooled stream already holds a split-K buffer"
    s = fresh[0]
    gen = torch.Generator().manual_seed(3)
    x, dy = torch.randn(2048, 256, generator=gen).cuda(), torch.randn(2048, 128, generator=gen).cuda()
    w, bias = torch.randn(128, 256, generator=gen).cuda(), torch.zeros(128).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        before = _scratch_info(s)
        try:
            L.check(lib.vog_train_pin_scratch(s.cuda_stream, 1), "vog_train_pin_scratch")
            assert before == (None, 0, 0)
            with pytest.raises(L.VogError, match="pinned"):
                BW.linear_f32(x, w, bias, False, dy=dy)
            assert _scratch_info(s) == (None, 0, 1)
            L.check(lib.vog_train_pin_scratch(s.cuda_stream, 0), "vog_train_pin_scratch")
            ref = BW.linear_f32(x, w, bias, False, dy=dy)["g_w"]
            s.synchronize()
            grown = _scratch_info(s)
            assert grown[0] is not None and grown[1] >= 8 * 128 * 256 * 4 and grown[2] == 0
            L.check(lib.vog_train_pin_scratch(s.cuda_stream, 1), "vog_train_pin_scratch")
            again = BW.linear_f32(x, w, bias, False, dy=dy)["g_w"]
            s.synchronize()
            assert _scratch_info(s) == (grown[0], grown[1], 1) and torch.equal(ref, again)
            want = dy.double().t() @ x.double()
            assert float((ref.double() - want).abs().max()) <= 1e-3 * float(want.abs().max())
        finally:
            lib.vog_train_pin_scratch(s.cuda_stream, 0)


# ---------------------------------------------------------------- trainer level
def _trainer(built, **kw):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = built
    return trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, **kw)


def _batches(dev):
    """The built batch and a second one with the features scaled by 0.5; the width of the word mask = the T of both sides."""
    half = {k: (v * 0.5 if k in ("pad_region_feature", "seg_feature_for_frms") else v.clone()) for k, v in dev.items()}
    return [dev, half], int(dev["srl_arg_word_mask"].shape[-1])


def _equal_state(a, b, what):
    assert set(a.m) == set(b.m) and a.m, what
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), (what, "p", k)
    for d, e, nm in ((a.m, b.m, "m"), (a.v, b.v, "v"), (a.vmax, b.vmax, "vmax"), (a.avg, b.avg, "avg")):
        assert set(d) == set(e), (what, nm)
        for k in d:
            assert torch.equal(d[k], e[k]), (what, nm, k)
    assert (a.num_it, a.adam_step) == (b.num_it, b.adam_step), what


def _four_steps(name, kw, between=None, what=""):
    """Four eager steps against a capture and four replays, on two alternating batches, both with T = the mask width."""
    built = _build(name)
    eager, graph = _trainer(built, **kw), _trainer(built, **kw)
    bs, W = _batches(built[6])
    slot = graph.capture(bs[0], T=W)
    assert graph.num_it == 0 and graph.adam_step == 0 and slot.T == W
    for k in graph.params:
        assert torch.equal(graph.params[k], eager.params[k]), k         # the capture's warm-up updates nothing
    want = []
    for i in range(4):
        if between is not None and i == 2:
            between(eager), between(graph)
        ld = eager.step(bs[i % 2], T=W)
        want.append({k: v.clone() for k, v in ld.items()})
        assert slot.step(bs[i % 2], longest=W) is None
    got = slot.losses(4)
    slot.check()
    for i in range(4):
        for k in eager.loss_fn.loss_keys:
            assert torch.equal(want[i][k].cpu(), got[i][k]), (what, i, k, float(want[i][k]), float(got[i][k]))
    assert any(float(want[0]["loss"]) != float(want[i]["loss"]) for i in (1, 2, 3))
    _equal_state(eager, graph, what)
    assert slot.replays == 4 and graph.num_it == 4
    return eager, graph, slot


MODES = {
    "plain fp32": dict(),
    "dropout": dict(dropout=True, dropout_seed=2 ** 45 + 11),           # (a seed baked in at capture fails from step 2 on)
    "clip": dict(clip_norm=1.0),
    "ema": dict(avg="ema", avg_decay=0.9),
    "frozen enc + lang": dict(freeze="enc,lang"),
    "opt-ins fp32": dict(attn="fused_pipe", lstm="fused", qkv="factored"),
    "opt-ins bf16": dict(amp="bf16", attn="fused_pipe", lstm="fused", qkv="factored", lstm_amp="split", gemm_amp="pipe"),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_four_replays_equal_four_eager_steps(mode):
    eager, graph, slot = _four_steps(NAME, MODES[mode], what=mode)
    if mode == "ema":
        assert graph.avg_state() == eager.avg_state() and eager.avg_state()["n_averaged"] == 4
    if mode == "frozen enc + lang":
        assert graph.frozen and not any(k in graph.m for k in graph.frozen)
    if mode == "dropout":                                                # and the masks do move from step to step
        fixed = _trainer(_build(NAME), dropout=True, dropout_seed=2 ** 45 + 11)
        bs, W = _batches(_build(NAME)[6])
        a = float(fixed.gradients(bs[0], T=W)[0]["loss"])
        fixed.num_it = 2
        assert a != float(fixed.gradients(bs[0], T=W)[0]["loss"])


def test_sep_model_with_the_verb_loss_in_the_ring():
    eager, graph, slot = _four_steps(SEP, dict(dropout=True), what="sep")
    assert slot.loss_keys == ["loss", "mdl_out_loss", "verb_loss"]


def test_dynamic_loss_scale_under_f16_skips_on_both_sides():
    eager, graph, slot = _four_steps(NAME, dict(amp="f16", loss_scale="dynamic"), what="f16 dynamic")
    se, sg = eager.scaler_state(), graph.scaler_state()
    print("scaler state after four steps:", se)
    assert repr(se) == repr(sg) and se["skipped"] >= 1 and se["adam_step"] + se["skipped"] == 4
    assert graph.adam_step == eager.adam_step == se["adam_step"]


def test_adamw_amsgrad_two_groups_and_a_moved_learning_rate():
    groups = [{"params": ["mult_txf", "lin2"], "lr": 2e-4, "weight_decay": 0.01},
              {"params": ["prop_encoder", "seg_encoder"], "weight_decay": 0.1}]
    eager, graph, slot = _four_steps(NAME, dict(optimizer="adamw", amsgrad=True, param_groups=groups),
                                     between=lambda t: t.set_lr(5e-5, [7e-5, 3e-5]), what="adamw amsgrad")
    assert graph.group_lrs() == [7e-5, 3e-5] and slot._lrs == [7e-5, 3e-5] and graph.vmax
    assert slot.lr_table.cpu().tolist() == [float(np.float32(7e-5)), float(np.float32(3e-5))]


def test_replays_allocate_nothing_and_an_eager_step_in_between_resynchronises():
    """Replays queued back to back, with another trainer's eager steps queued straight behind them and no host wait in
    between; then a slot whose trainer stepped eagerly between two replays."""
    built = _build(NAME)
    eager, graph = _trainer(built, dropout=True), _trainer(built, dropout=True)
    bs, W = _batches(built[6])
    slot = graph.capture(bs[0], T=W)
    slot.step(bs[0])
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for i in (1, 0, 1):
        slot.step(bs[i])
        assert torch.cuda.memory_allocated() == mem
    for i in (0, 1, 0, 1):
        eager.step(bs[i], T=W)
    _equal_state(eager, graph, "four replays")
    # replay, eager, eager, replay: the slot rewrites its counts from the trainer's
    eager, graph = _trainer(built, dropout=True), _trainer(built, dropout=True)
    slot = graph.capture(bs[0], T=W)
    slot.step(bs[0])
    graph.step(bs[1], T=W)
    graph.step(bs[0], T=W)
    slot.step(bs[1])
    for i in (0, 1, 0, 1):
        eager.step(bs[i], T=W)
    _equal_state(eager, graph, "replay, eager, eager, replay")
    assert [sorted(d) for d in slot.losses(2)] == [sorted(eager.loss_fn.loss_keys)] * 2 and slot._ticks == [0, 3]
    with pytest.raises(L.VogError, match="holds the last 2"):
        slot.losses(3)


def test_stale_slots_and_long_sentences_are_refused_before_any_launch():
    built = _build(NAME)
    tr = _trainer(built)
    bs, W = _batches(built[6])
    slot = tr.capture(bs[0], T=W)
    before = {k: v.clone() for k, v in tr.params.items()}
    with pytest.raises(ValueError, match="longest"):
        slot.step(bs[0], longest=W + 1)
    short = {k: v[:1] if v.shape[0] == 2 else v for k, v in bs[0].items()}
    with pytest.raises(L.VogError, match="stale"):
        slot.step(short)
    tr.set_param_groups(None)
    with pytest.raises(L.VogError, match="stale"):
        slot.step(bs[0])
    torch.cuda.synchronize()
    assert tr.num_it == 0 and slot.replays == 0 and all(torch.equal(tr.params[k], before[k]) for k in before)
    tr.capture(bs[0], T=W).step(bs[0])                                  # captured again, it runs
    assert tr.num_it == 1
    with pytest.raises(L.VogError, match="accum_steps"):
        _trainer(built, accum_steps=2).capture(bs[0])
    with pytest.raises(ValueError, match="T = "):
        tr.capture(bs[0], T=W + 1)


def test_a_length_beyond_t_is_clamped_and_reported():
    built = _build(NAME)
    tr = _trainer(built)
    bs, W = _batches(built[6])
    longest = int(bs[0]["srl_arg_word_mask_len"].max())
    assert longest >= 2
    slot = tr.capture(bs[0], T=longest - 1)
    slot.step(bs[0])
    assert int(slot.static["srl_arg_word_mask_len"].max()) == longest - 1
    with pytest.raises(L.VogError, match="clamped"):
        slot.check()
    assert all(bool(torch.isfinite(v).all()) for v in tr.params.values())


def test_padded_t_against_the_exact_longest_length():
    """A slot captured with T = the mask width against eager steps that read the longest length: the language kernels run over
    more positions, all of them past every sentence's end, where states are frozen and gradients zero. Without dropout that
    changes no bit (with dropout the mask indices depend on T): losses, parameters and moments after three steps are equal."""
    built = _build(NAME)
    eager, graph = _trainer(built), _trainer(built)
    bs, W = _batches(built[6])
    longest = int(bs[0]["srl_arg_word_mask_len"].max())
    slot = graph.capture(bs[0], T=W)
    want = []
    for i in range(3):
        want.append(float(eager.step(bs[i % 2])["loss"]))
        slot.step(bs[i % 2])
    got = [float(d["loss"]) for d in slot.losses(3)]
    dl = max(abs(a - b) for a, b in zip(want, got))
    dp = max(float((eager.params[k] - graph.params[k]).abs().max()) / max(float(eager.params[k].abs().max()), 1e-30) for k in eager.params)
    print(f"T = {W} against the longest length {longest}: loss diff {dl:.3e}, parameters rel diff {dp:.3e}")
    assert W > longest
    assert want == got                                                  # without dropout the padded positions change no bit
    _equal_state(eager, graph, "padded T")


def _learner(tmp_path, uid, graph):
    torch.manual_seed(1234)
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    comm = comm_for(c)
    B, ncmp = batch["num_cmp_msk"].shape
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    # both runs with the same T: the first sentence fills the mask, so the eager step's longest length is the slot's T
    W = one["srl_arg_word_mask"].shape[-1]
    one["srl_arg_word_mask_len"].view(-1)[0] = W
    one["srl_arg_word_mask"].view(-1, W)[0] = 1
    half = {k: (v * 0.5 if k in ("pad_region_feature", "seg_feature_for_frms") else v) for k, v in one.items()}
    tail = {k: v[:1] for k, v in one.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one, half, one, tail], valid_dl=[one], test_dl=[one])
    cfg.hip.train_graph = graph
    evl = sel_mod.get_mdl_loss_eval(cfg)["eval"](cfg, comm, torch.device("cuda", 0))
    return tu.Learner(uid=uid, data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)


def test_learner_replays_the_epochs_shape_and_falls_back_for_the_tail(tmp_path):
    runs = {}
    for graph in (False, True):
        learn = _learner(tmp_path / str(graph), "g" if graph else "e", graph)
        learn.trainer.set_param_groups(None)
        smooth = [learn.train_epoch() for _ in range(2)]
        runs[graph] = (learn, smooth)
    (le, se), (lg, sg) = runs[False], runs[True]
    assert (lg.graph_replays, lg.graph_fallbacks) == (6, 2) and (le.graph_replays, le.graph_fallbacks) == (0, 0)
    assert le.train_slot is None and lg.train_slot is not None and lg.num_it == le.num_it == 8
    _equal_state(le.trainer, lg.trainer, "learner")
    assert se == sg, (se, sg)                                            # fp32 ring rows, smoothed in iteration order: the same floats
    hist = lg.fit(1, lr=1e-4)                                            # fit drops the slot with the groups and captures again
    assert len(hist) == 1 and lg.graph_replays == 9 and lg.graph_fallbacks == 3
