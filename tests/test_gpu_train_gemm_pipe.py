"""The pipelined 16-bit tile GEMM of the training path (`vog_train_set_int("gemm_amp_pipe", 1)` under "amp":
gemm16_pipe_kernel<T, MI, NJ> in csrc/train_gemm.hip) on the device. Its contract is the tile kernel's bits: the same operands,
rounding, MFMA, order of the 32-wide chunks and epilogue, so every comparison with gemm16_kernel<T, false> is `torch.equal`.
Operator level (vog_linear_f32: three operand layouts, split-K; vog_attn_f32: batches), one anchor against the rounded float64
restatement of tests/test_gpu_train_ops.py::test_linear_skinny_amp, the switch's isolation from fp32 and from the scalar form, and
the switch through the trainer, the autograd path and the Learner. Every test sets the switch in a try / finally that resets it."""
import contextlib
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_amp import _sd
from tests.test_gpu_train_ops import F64, _ShortBy1, attn_call, close, dev, guarded, linear_call

pytestmark = pytest.mark.gpu
bwd = importlib.import_module("vognet-pytorch_amd.backward")
L = bwd.L
AMPS = [(1, torch.bfloat16), (2, torch.float16)]
AMP_IDS = ["bf16", "f16"]


def _get(name):
    v = C.c_int(-7)
    assert L.load().vog_train_get_int(name, C.byref(v)) == 0
    return v.value


@contextlib.contextmanager
def amp_pipe(on=1, amp=1):
    """The calling thread's switches for the calls inside, reset behind them; both launch counters start at 0."""
    lib = L.load()
    try:
        assert lib.vog_train_set_int(b"gemm_amp_pipe", on) == 0
        assert lib.vog_train_set_int(b"amp", amp) == 0
        assert lib.vog_train_set_int(b"gemm_amp_pipe_launches", 0) == 0
        assert lib.vog_train_set_int(b"f32_products", 0) == 0
        yield
    finally:
        lib.vog_train_set_int(b"gemm_amp_pipe", 0)
        lib.vog_train_set_int(b"amp", 0)


# ---- 1. vog_linear_f32: bit equality with the tile kernel ----------------------------------------------------------------------
# The three products of vog_linear_f32(M, N, K), dims as [M', N', K'] (tests/test_gpu_train_ops.py::LIN_CASES derives the branches):
#   y   = x W^T     [M, N, K]  A row-major, B = W with bk = 1     (both operands k-contiguous)
#   g_w = dpre^T x  [N, K, M]  A column-major, B row-major        (both operands row-contiguous: 4 x (ROWS / 16) blocks per thread)
#   d_x = dpre W    [M, K, N]  A row-major, B row-major
# The counter counts launches of gemm16_pipe_kernel: one per product that reaches the vector tile, one per split-K product (its
# partials are ONE launch over blockIdx.z; the reduction is another kernel), none for the weight-stream kernel (y with M <= 16 and
# N >= 256). There is one tile instantiation, <2, 2> (64 x 64), and every case reaches it. The pipeline holds one 64-wide episode
# in LDS ahead of the MFMAs and one in registers (depth 2), so prologue, steady state and drain all run from K' > 3 * 64 = 192 on.
PIPE_LIN = [
    # M, N, K, options, launches                  what it reaches (every product on the one instantiation, <2, 2>)
    (4, 4, 4, {}, 3),                             # one partial chunk, one partial tile
    (64, 32, 48, {}, 3),                          # one and a half chunks: one episode whose second k-step is partial
    (132, 68, 36, {}, 3),                         # partial tiles in both dimensions of all three products (132 = 2 * 64 + 4, 68 = 64 + 4)
    (260, 200, 292, {}, 3),                       # K' = 292 / 260 / 200: 5 / 5 / 4 episodes with tails of 36 / 4 / 8; several tiles
    (64, 32, 32, {}, 3),                          # K' = 32 (y): one episode, second k-step skipped; 64 (g_w): one full episode
    (64, 32, 64, {}, 3),                          # K' = 64 (y, g_w): one full episode, nothing to prefetch
    (2048, 8, 12, {"acc"}, 3),                    # g_w: vector split-K, K' = 2048 in 8 chunks of 256 (grid z = 8); d_x accumulates
    (1040, 8, 12, {}, 3),                         # g_w: split-K with kchunk = 272: block starts 272 z (no multiples of 32), 4 episodes + a
                                                  # 16-wide k-step per block, last block 224
    (8, 1024, 12, {"acc"}, 2),                    # y is the weight-stream kernel (not counted); d_x: split-K (K' = 1024), accumulating
    (2048, 1024, 196, {}, 3),                     # grids of more workgroups than the chip has CUs: y 16 x 32 tiles; g_w 4 x 16 tiles x
                                                  # 8 chunks of 256; d_x 4 x 32 tiles x 4 chunks of 256; y: 4 episodes, tail 4
]


def _lin_inputs(M, N, K, col0):
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    dy = torch.randn(M, N + 8, generator=g)                            # the layer's output gradient sits inside a wider matrix
    prefill = torch.randn(M, K, generator=g)
    return dev(x), dev(w), dev(b), dev(dy), prefill, col0


def _lin_run(inp, on, amp, acc, relu=True):
    x, w, b, dy, prefill, col0 = inp
    with amp_pipe(on, amp):
        r = linear_call(x, w, b, relu, dy=dy, dy_col0=col0, want_y=True, want_dx=True, d_x=dev(prefill) if acc else None)
        torch.cuda.synchronize()
        return r, _get(b"gemm_amp_pipe_launches"), _get(b"f32_products")


@pytest.mark.parametrize("amp", [1, 2], ids=AMP_IDS)
@pytest.mark.parametrize("M,N,K,opts,launches", PIPE_LIN)
def test_linear_bits_equal_the_tile_kernel(M, N, K, opts, launches, amp):
    inp = _lin_inputs(M, N, K, 4 if M % 8 else 0)                      # aligned dy: column 0 or 4
    tile, n_tile, _ = _lin_run(inp, 0, amp, "acc" in opts)
    pipe, n_pipe, n32 = _lin_run(inp, 1, amp, "acc" in opts)
    assert n_tile == 0 and n_pipe == launches and n32 == 0
    for k in ("y", "g_w", "g_b", "d_x"):
        assert torch.isfinite(pipe[k]).all() and torch.equal(pipe[k], tile[k]), k


# ---- 2. vog_attn_f32: batched vector calls ---------------------------------------------------------------------------------------
# d = 24 in 3 heads of 8, N = 12 tokens (4 proposals x 3), S = 3 sequences: every per-head product (dims 12 x 12 x 8, 12 x 8 x 12,
# operands at column offsets 8 h, batch strides 12 * 24 and 12 * 12) stays vector and runs over blockIdx.z = 3.
# Forward call: 3 projections + per head (logits, O_h) = 3 + 3 * 2 = 9 launches. Backward call: 3 projections + per head (logits,
# dV_h, d drop(P), dQ_h, dK_h) + 3 weight gradients + 3 d_x = 3 + 3 * 5 + 3 + 3 = 24.
@pytest.mark.parametrize("amp", [1, 2], ids=AMP_IDS)
def test_attention_batched_bits_equal_the_tile_kernel(amp):
    S, n, nsrl, d, H = 3, 4, 3, 24, 3
    N = n * nsrl
    g = torch.Generator().manual_seed(5)
    x, d_cat = dev(torch.randn(S * N, d, generator=g)), dev(torch.randn(S * N, d, generator=g))
    w = {k: dev(torch.randn(d, d, generator=g) / math.sqrt(d)) for k in ("wq", "wk", "wv")}
    props = dev(torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.]))
    pe = (dev(torch.randn(H, 5, generator=g)), dev(torch.randn(H, generator=g) * 0.3))
    boxes = bwd._Boxes(props, 720.0, 405.0, 10.0)
    got = {}
    for on in (0, 1):
        with amp_pipe(on, amp):
            f = attn_call(w, pe, x, S, N, n, H, boxes)
            nf = _get(b"gemm_amp_pipe_launches")
            r = attn_call(w, pe, x, S, N, n, H, boxes, d_cat=d_cat)
            torch.cuda.synchronize()
            got[on] = (f, r, nf, _get(b"gemm_amp_pipe_launches") - nf)
    assert got[0][2:] == (0, 0) and got[1][2:] == (9, 24)
    assert torch.equal(got[0][0]["cat"], got[1][0]["cat"])
    for k in ("g_wq", "g_wk", "g_wv", "g_pe_w", "g_pe_b", "d_x"):
        assert torch.isfinite(got[1][1][k]).all() and torch.equal(got[0][1][k], got[1][1][k]), k


# ---- 3. one independent anchor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp,dt", AMPS, ids=AMP_IDS)
def test_forward_against_the_rounded_restatement(amp, dt):
    """relu(x16 @ w16^T + b) in float64, operands rounded as tests/test_gpu_amp.py rounds them, under test_linear_skinny_amp's bound
    (a product of two 16-bit values is exact in fp32; K = 292 fp32 additions stay orders below it)."""
    M, N, K = 260, 200, 292
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    y = torch.relu(x.to(dt).to(F64) @ w.to(dt).to(F64).t() + b.to(F64))
    with amp_pipe(1, amp):
        f = linear_call(dev(x), dev(w), dev(b), True)
        assert _get(b"gemm_amp_pipe_launches") == 1 and _get(b"f32_products") == 0
    close(f["y"], y, what=f"y (amp = {amp}, pipe)")


# ---- 4. switch discipline ---------------------------------------------------------------------------------------------------------
def test_without_amp_the_switch_changes_nothing():
    inp = _lin_inputs(260, 200, 292, 4)
    off, n_off, f_off = _lin_run(inp, 0, 0, False)
    on, n_on, f_on = _lin_run(inp, 1, 0, False)
    assert n_off == 0 and n_on == 0 and f_off == f_on == 3              # the three fp32 tile launches, with and without the switch
    for k in ("y", "g_w", "g_b", "d_x"):
        assert torch.equal(on[k], off[k]), k
    assert _get(b"gemm_amp_pipe") == 0 and _get(b"amp") == 0


@pytest.mark.parametrize("amp", [1, 2], ids=AMP_IDS)
@pytest.mark.parametrize("col0", [0, 3])
def test_scalar_form_stays_with_the_scalar_tile(col0, amp):
    """(33, 7, 9): odd dimensions and strides, every product is the element-wise tile, whatever the column of dy."""
    inp = _lin_inputs(33, 7, 9, col0)
    tile, n_tile, _ = _lin_run(inp, 0, amp, True)
    pipe, n_pipe, n32 = _lin_run(inp, 1, amp, True)
    assert n_tile == 0 and n_pipe == 0 and n32 == 0
    for k in ("y", "g_w", "g_b", "d_x"):
        assert torch.equal(pipe[k], tile[k]), k


@pytest.mark.parametrize("amp", [1, 2], ids=AMP_IDS)
def test_misaligned_dy_keeps_its_bits(amp):
    """dy at column 3 of its matrix (12 bytes off a 16-byte boundary): dy is read by the row kernel that writes dpre into the
    scratch, never by a product, so the three products stay vector; the bits are the tile kernel's."""
    inp = _lin_inputs(132, 68, 36, 3)
    tile, n_tile, _ = _lin_run(inp, 0, amp, False)
    pipe, n_pipe, _ = _lin_run(inp, 1, amp, False)
    assert n_tile == 0 and n_pipe == 3
    for k in ("y", "g_w", "g_b", "d_x"):
        assert torch.equal(pipe[k], tile[k]), k


def test_two_runs_give_the_same_bits():
    inp = _lin_inputs(2048, 8, 12, 0)
    a, na, _ = _lin_run(inp, 1, 1, True)
    b, nb, _ = _lin_run(inp, 1, 1, True)
    assert na == nb == 3
    for k in ("y", "g_w", "g_b", "d_x"):
        assert torch.equal(a[k], b[k]), k


def test_a_scratch_one_byte_short_is_refused_before_any_launch(monkeypatch):
    lib = L.load()
    monkeypatch.setattr(bwd.L, "load", lambda: _ShortBy1(lib, "vog_linear_f32_scratch_bytes"))
    g = torch.Generator().manual_seed(1)
    z = lambda *s: torch.randn(*s, generator=g).cuda()
    try:
        assert lib.vog_train_set_int(b"amp", 1) == 0 and lib.vog_train_set_int(b"gemm_amp_pipe", 1) == 0
        assert lib.vog_train_set_int(b"gemm_amp_pipe_launches", 0) == 0
        with pytest.raises(L.VogError, match="rc=-2"):
            bwd.linear_f32(z(4, 8), z(8, 8), z(8), True)
        n = C.c_int(-7)
        assert lib.vog_train_get_int(b"gemm_amp_pipe_launches", C.byref(n)) == 0 and n.value == 0
    finally:
        lib.vog_train_set_int(b"amp", 0)
        lib.vog_train_set_int(b"gemm_amp_pipe", 0)


# ---- 5. through the trainer, the autograd path and the Learner ------------------------------------------------------------------
from tests.gpu_util import comm_for                                         # noqa: E402
from tests.test_gpu_autograd import _build, _grads                          # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
NAME = "small/vog_spat"


def test_trainer_refuses_another_string():
    cfg, sd, batch, tg, c, mdl, dev_b, loss_fn = _build(NAME)
    for bad in ("Pipe", "split", None):
        with pytest.raises(ValueError, match="gemm_amp"):
            trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16", gemm_amp=bad)
    assert trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp="bf16").gemm_amp == "tile"


@pytest.mark.parametrize("amp", ["bf16", "f16"])
def test_three_adam_steps_give_the_default_amp_trainers_parameters(amp):
    cfg, sd, batch, tg, c, mdl, dev_b, loss_fn = _build(NAME)
    tp = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp=amp, gemm_amp="pipe")
    tt = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, amp=amp)
    assert L.load().vog_train_set_int(b"gemm_amp_pipe_launches", 0) == 0
    lt = [float(tt.step(dev_b)["loss"]) for _ in range(3)]
    assert _get(b"gemm_amp_pipe_launches") == 0                              # the default never reaches the new kernel
    lp = [float(tp.step(dev_b)["loss"]) for _ in range(3)]
    assert _get(b"gemm_amp_pipe_launches") > 0 and _get(b"gemm_amp_pipe") == 0 and _get(b"amp") == 0
    assert lp == lt, (lp, lt)
    for k, v in tt.params.items():
        assert torch.equal(tp.params[k], v), k


def test_autograd_path_takes_the_switch_from_the_cfg():
    cfg, sd, batch, tg, c, mdl, dev_b, loss_fn = _build(NAME)
    mdl.eval().requires_grad_(True)
    got = {}
    for mode in ("tile", "pipe"):
        cfg.hip.train_gemm_amp = mode
        mdl.zero_grad(set_to_none=True)
        assert L.load().vog_train_set_int(b"gemm_amp_pipe_launches", 0) == 0
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ld = loss_fn(mdl(dev_b), dev_b)
        ld["loss"].backward()
        n = _get(b"gemm_amp_pipe_launches")
        assert (n > 0) == (mode == "pipe") and _get(b"gemm_amp_pipe") == 0 and _get(b"amp") == 0
        got[mode] = {k: v.clone() for k, v in _grads(mdl).items()}
    assert set(got["tile"]) == set(got["pipe"]) and got["tile"]
    for k, v in got["tile"].items():
        assert torch.equal(got["pipe"][k], v), k


def test_learner_trains_pipe_and_its_checkpoint_loads_into_the_default(tmp_path):
    cfg, sd, batch, tg, c, mdl, dev_b, loss_fn = _build(NAME)
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    comm = comm_for(c)
    B, ncmp = batch["num_cmp_msk"].shape
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one, one], valid_dl=[one], test_dl=[one])
    cfg.hip.train_amp = "bf16"
    cfg.hip.train_gemm_amp = "pipe"
    evl = sel_mod.get_mdl_loss_eval(cfg)["eval"](cfg, comm, torch.device("cuda", 0))
    learn = tu.Learner(uid="P0", data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)
    assert learn.trainer.amp == "bf16" and learn.trainer.gemm_amp == "pipe"
    assert L.load().vog_train_set_int(b"gemm_amp_pipe_launches", 0) == 0
    hist = learn.fit(epochs=1, lr=1e-4)
    assert len(hist) == 1 and np.isfinite(hist[0]["trn_loss"]) and learn.num_it == 2
    assert _get(b"gemm_amp_pipe_launches") > 0 and _get(b"gemm_amp_pipe") == 0 and _get(b"amp") == 0
    learn.save_model_dict()
    cfg2, sd2, _, _, _, mdl2, _, loss2 = _build(NAME)
    assert cfg2.hip.train_gemm_amp == "tile" and cfg2.hip.train_amp == ""
    learn2 = tu.Learner(uid="P0", data=data, mdl=mdl2, loss_fn=loss2, cfg=cfg2,
                        eval_fn=sel_mod.get_mdl_loss_eval(cfg2)["eval"](cfg2, comm, torch.device("cuda", 0)), comm=comm)
    assert learn2.trainer.gemm_amp == "tile" and learn2.trainer.amp is None
    for k, v in learn.trainer.state_dict().items():
        assert torch.equal(v, learn2.trainer.params[k]), k
    assert learn2.trainer.num_it == 2
