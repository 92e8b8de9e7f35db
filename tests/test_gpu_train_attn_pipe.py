"""The pipelined kernels of the fused training attention (`vog_train_set_int("attn_fused_pipe", 1)`: fa_fwd_pipe_kernel,
fa_bwd_q_pipe_kernel, fa_bwd_kv_pipe_kernel in csrc/train_attn.hip: fa_fwd_body, fa_bwd_q_body, fa_bwd_kv_body under the
StreamPipe policy) on the device. Their contract is the bits of the plain fused kernels (the same bodies under StreamPlain,
but for the plain dQ kernel, which is written out and so is held to fa_bwd_q_body only by these tests) - the same sub-tile, MFMAs, assignment of k to lanes, rounding points and summation orders - so every comparison here is
`torch.equal` against a call with the switch off; accuracy against autograd and the rounded restatement is asserted for the plain
kernels in tests/test_gpu_train_attn.py. Every operator call runs on a scratch of exactly `vog_attn_fused_scratch_bytes` between
two guard bands, at both shifts of the base. Every test sets the switch in a try / finally that resets it.

Staged tiles are KT = 64 rows (fp32 at head sizes above 128: 32), sub-tiles 16 (fp32) / 32 (16-bit) rows, a workgroup owns 64
rows: the N of F32_SHAPES sit on and around every one of these boundaries and give 1, 2, 3 and more tiles."""
import contextlib
import ctypes as C
import importlib

import pytest
import torch

from tests.test_gpu_amp import _sd, _switch, MODES
from tests.test_gpu_train_attn import GRADS, _case, _dev, fused_call

pytestmark = pytest.mark.gpu
bwd = importlib.import_module("vognet-pytorch_amd.backward")
L = bwd.L
SHIFTS = (1, 252)
DROPS = [None, (0.2, 77, 210)]
F32_SHAPES = ([(2, 1, 1, 8, 2, True), (1, 9, 2, 20, 4, False)] +
              [(2, N, 1, 48, 3, True) for N in (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 257, 300)] +
              [(3, 100, 1, 512, 3, True), (2, 20, 5, 768, 3, True), (1, 400, 5, 96, 3, True)])
AMP_SHAPES = [(3, 7, 2, 32, 3), (2, 65, 1, 64, 2), (2, 20, 1, 512, 3), (2, 20, 5, 768, 3), (2, 129, 1, 48, 3), (1, 400, 5, 96, 3)]


@contextlib.contextmanager
def pipe(on=1, amp=0):
    """The calling thread's switches for the calls inside, reset behind them; both launch counters start at 0."""
    lib = L.load()
    try:
        assert lib.vog_train_set_int(b"attn_fused_pipe", on) == 0
        assert lib.vog_train_set_int(b"amp", amp) == 0
        assert lib.vog_train_set_int(b"attn_fused_pipe_launches", 0) == 0
        assert lib.vog_train_set_int(b"f32_products", 0) == 0
        yield
    finally:
        lib.vog_train_set_int(b"attn_fused_pipe", 0)
        lib.vog_train_set_int(b"amp", 0)


def _run(c, on, amp, drop, shift):
    """Forward, stand-alone backward and kept-forward backward -> (results, launches of the pipelined kernels per call,
    fp32 product launches per call)."""
    args, dc = _dev(c)
    with pipe(on, amp):
        marks = [(_switch(b"attn_fused_pipe_launches"), _switch(b"f32_products"))]
        f = fused_call(*args, shift=shift, drop=drop)
        marks.append((_switch(b"attn_fused_pipe_launches"), _switch(b"f32_products")))
        alone = fused_call(*args, shift=shift, d_cat=dc, drop=drop)
        marks.append((_switch(b"attn_fused_pipe_launches"), _switch(b"f32_products")))
        kept = fused_call(*args, shift=shift, d_cat=dc, drop=drop, lse=f["lse"], cat=f["cat"])
        marks.append((_switch(b"attn_fused_pipe_launches"), _switch(b"f32_products")))
        torch.cuda.synchronize()
    steps = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(marks, marks[1:])]
    return (f, alone, kept), [s[0] for s in steps], [s[1] for s in steps]


def _same_bits(c, amp, drop, shift):
    (f0, a0, k0), n0, p0 = _run(c, 0, amp, drop, shift)
    (f1, a1, k1), n1, p1 = _run(c, 1, amp, drop, shift)
    assert n0 == [0, 0, 0] and n1 == [1, 3, 2], (n0, n1)        # forward | forward, dQ, dK / dV | dQ, dK / dV
    assert p0 == p1, (p0, p1)                                   # fp32 product launches move as they do for "fused"
    if amp:
        assert p1 == [0, 0, 0]
    for k in ("cat", "lse"):
        assert torch.isfinite(f1[k]).all() and torch.equal(f0[k], f1[k]), k
    for k in GRADS:
        assert (k in a0) == (k in a1) and (k in k0) == (k in k1), k
        if k in a0:
            assert torch.isfinite(a1[k]).all() and torch.equal(a0[k], a1[k]), ("stand-alone", k)
            assert torch.equal(k0[k], k1[k]), ("kept forward", k)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("drop", DROPS, ids=["nodrop", "drop"])
@pytest.mark.parametrize("S,n,nsrl,d,H,rel", F32_SHAPES)
def test_fp32_bits_equal_the_fused_kernels(S, n, nsrl, d, H, rel, drop, shift):
    _same_bits(_case(S, n, nsrl, d, H, rel), 0, drop, shift)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("drop", DROPS, ids=["nodrop", "drop"])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("S,n,nsrl,d,H", AMP_SHAPES)
def test_amp_bits_equal_the_fused_kernels(S, n, nsrl, d, H, mode, drop, shift):
    _same_bits(_case(S, n, nsrl, d, H, True), MODES[mode][1], drop, shift)


def test_counters():
    c = _case(2, 65, 1, 64, 2, True)
    args, dc = _dev(c)
    with pipe(1, 0):
        f = fused_call(*args)
        assert _switch(b"attn_fused_pipe_launches") == 1
        n32 = _switch(b"f32_products")
        fused_call(*args, d_cat=dc)
        assert _switch(b"attn_fused_pipe_launches") == 4
        fused_call(*args, d_cat=dc, lse=f["lse"], cat=f["cat"])
        assert _switch(b"attn_fused_pipe_launches") == 6
        on32 = (n32, _switch(b"f32_products"))
    with pipe(0, 0):
        f = fused_call(*args)
        n32 = _switch(b"f32_products")
        fused_call(*args, d_cat=dc)
        fused_call(*args, d_cat=dc, lse=f["lse"], cat=f["cat"])
        assert _switch(b"attn_fused_pipe_launches") == 0            # "fused" never reaches the new kernels
        assert (n32, _switch(b"f32_products")) == on32 and n32 > 0
    with pipe(1, 1):
        fused_call(*args, d_cat=dc)
        assert _switch(b"attn_fused_pipe_launches") == 3 and _switch(b"f32_products") == 0
    torch.cuda.synchronize()
    assert _switch(b"attn_fused_pipe") == 0 and _switch(b"amp") == 0


@pytest.mark.parametrize("amp", [0, 1])
def test_two_pipe_calls_give_the_same_bits(amp):
    c = _case(2, 129, 1, 48, 3, True)
    a, na, _ = _run(c, 1, amp, (0.2, 77, 210), 1)
    b, nb, _ = _run(c, 1, amp, (0.2, 77, 210), 1)
    assert na == nb == [1, 3, 2]
    for x, y in zip(a, b):
        for k in ("cat", "lse") + GRADS:
            if k in x:
                assert torch.equal(x[k], y[k]), k


# ---------------------------------------------------------------- the whole path: trainer, autograd
from tests.gpu_util import comm_for                                         # noqa: E402
from tests.test_gpu_autograd import _build, _grads                          # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")


def _three_steps(name, attn, **kw):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    t = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, **({} if attn is None else {"attn": attn}), **kw)
    assert L.load().vog_train_set_int(b"attn_fused_pipe_launches", 0) == 0
    losses = [float(t.step(dev)["loss"]) for _ in range(3)]
    torch.cuda.synchronize()
    n = _switch(b"attn_fused_pipe_launches")
    assert _switch(b"attn_fused_pipe") == 0 and _switch(b"amp") == 0         # precision() reset them
    return t, losses, n


@pytest.mark.parametrize("kw", [{}, {"amp": "bf16"}, {"dropout": True, "dropout_seed": 7}], ids=["fp32", "bf16", "dropout"])
@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep_cmpmsk"])
def test_three_adam_steps_give_the_fused_trainers_parameters(name, kw):
    tf, lf, nf = _three_steps(name, "fused", **kw)
    tp, lp, np_ = _three_steps(name, "fused_pipe", **kw)
    assert tp.attn == "fused_pipe" and tf.attn == "fused"
    assert nf == 0 and np_ > 0, (nf, np_)
    assert lp == lf, (lp, lf)
    for k, v in tf.params.items():
        assert torch.equal(tp.params[k], v), k


def test_default_trainer_leaves_the_counter_at_zero():
    t, losses, n = _three_steps("small/vog_spat", None)
    assert t.attn == "materialized" and n == 0


def test_switch_is_reset_when_the_step_raises(monkeypatch):
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    t = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, attn="fused_pipe")
    seen = []

    def boom(*a, **k):
        seen.append(_switch(b"attn_fused_pipe"))
        raise RuntimeError("stop here")

    monkeypatch.setattr(bwd, "_attn_call", boom)
    with pytest.raises(RuntimeError, match="stop here"):
        t.step(dev)
    assert seen == [1] and _switch(b"attn_fused_pipe") == 0


def test_autograd_path_takes_the_value_from_the_cfg():
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build("small/vog_spat")
    mdl.eval().requires_grad_(True)
    got, n = {}, {}
    for mode in ("fused", "fused_pipe"):
        cfg.hip.train_attn = mode
        mdl.zero_grad(set_to_none=True)
        assert L.load().vog_train_set_int(b"attn_fused_pipe_launches", 0) == 0
        loss_fn(mdl(dev), dev)["loss"].backward()
        torch.cuda.synchronize()
        n[mode] = _switch(b"attn_fused_pipe_launches")
        assert _switch(b"attn_fused_pipe") == 0
        got[mode] = {k: v.clone() for k, v in _grads(mdl).items()}
    assert n["fused"] == 0 and n["fused_pipe"] > 0, n
    assert set(got["fused"]) == set(got["fused_pipe"]) and got["fused"]
    for k, v in got["fused"].items():
        assert torch.equal(got["fused_pipe"][k], v), k
