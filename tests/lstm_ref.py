"""Reference of one BiLSTM layer for the operator tests of csrc/lstm.hip / lstm_dev.h, plain torch on the CPU.

`bilstm_ref` restates one bidirectional layer with packed-sequence semantics (nn.LSTM gate order i, f, g, o; zero initial
state; direction 1 visits position len-1-s at step s; zeros past each length; final hidden = [h_fwd(last active step) ||
h_bwd(last active step, i.e. position 0)]) as a ROUNDED restatement of what the kernels compute: W_hh (and for the fused form
W_ih and the layer input, see `project`) are rounded to the 16-bit type first, h is rounded to the 16-bit type after every
step - that rounded value is what travels to the next step and what is output - and gates, c and every sum are float64.
acc="f32perm" is the second accumulation mode: float32 throughout, the recurrent dot product summed over a permuted k order.
The tests use it only to measure the reference's own rounding-flip noise (how often two faithful evaluations of the same
recurrence land on different 16-bit neighbours).

The keyword arguments gate_order / dir1_pos (and final_from_last_step) exist for the deliberate-mutation checks of
test_lstm_ref_host.py: the defaults are the semantics above.

The other functions build the input forms the kernels take from the same (gates, weights) and list the case families that
tests/test_lstm_ref_host.py (conditions on the reference alone) and tests/test_gpu_lstm_ops.py (the kernels) share."""
import ctypes as C
import math
import zlib

import numpy as np
import torch

F64 = torch.float64
T16 = {"f16": torch.float16, "bf16": torch.bfloat16}
ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}           # spacing just below 1.0 (|h| < 1)
MAX_ULP = 2.0                                          # criterion (a)
SHARE_FACTOR, SHARE_FLOOR = 4.0, 0.01                  # criterion (b)


def round16(x, dtype):
    """x rounded to the 16-bit type (through float32, as the kernels round their fp32 values), in x's own type; None: x."""
    return x if dtype is None else x.to(torch.float32).to(T16[dtype]).to(x.dtype)


def prep_whh(w_hh, dtype, acc="f64", perm_seed=1):
    """w_hh [2][4R][R] rounded to the 16-bit type, in the accumulation type, transposed for the recurrent product and (acc =
    "f32perm") with its k axis permuted - made once per (weights, dtype, mode) and handed to bilstm_ref in place of w_hh."""
    R = w_hh.shape[2]
    F = F64 if acc == "f64" else torch.float32
    perm = torch.arange(R) if acc == "f64" else torch.randperm(R, generator=torch.Generator().manual_seed(perm_seed))
    w = round16(w_hh.to(F64), dtype).to(F)
    return {"F": F, "perm": perm, "wt": w[:, :, perm].transpose(1, 2).contiguous()}       # wt [2][R][4R]


def bilstm_ref(gx, w_hh, lens, dtype, acc="f64", gate_order=(0, 1, 2, 3), dir1_pos=None, h_noise=0.0, noise_seed=0):
    """gx [2][Bn][T][4R]: x W_ih^T + b_ih + b_hh per (direction, sentence, POSITION), gate-major 4R axis; w_hh [2][4R][R] or
    its prep_whh (which then decides the accumulation mode); lens [Bn]. -> out [Bn][T][2R], fin [Bn][2R], float64 holding
    exact 16-bit values (dtype None: no rounding anywhere). h_noise: relative perturbation (uniform in +-h_noise) of every h
    before it is rounded - the probes of `settled`."""
    _, Bn, T, R4 = gx.shape
    R = R4 // 4
    pw = w_hh if isinstance(w_hh, dict) else prep_whh(w_hh, dtype, acc)
    F, perm, wt = pw["F"], pw["perm"], pw["wt"]
    lens = torch.as_tensor(lens, dtype=torch.int64)
    g_in = gx.to(F)
    if dir1_pos is None:
        dir1_pos = lambda s, ln: ln - 1 - s                                 # noqa: E731
    h = torch.zeros(2, Bn, R, dtype=F)
    c = torch.zeros(2, Bn, R, dtype=F)
    out = torch.zeros(Bn, T, 2 * R, dtype=F64)
    rows = torch.arange(Bn)
    gi, gf, gg, go = gate_order
    ng = torch.Generator().manual_seed(noise_seed)
    for s in range(min(T, int(lens.max()))):
        act = lens > s
        pos = torch.stack([torch.full_like(lens, s), dir1_pos(s, lens)]).clamp(0, T - 1)   # [2][Bn]
        gates = torch.stack([g_in[d, rows, pos[d]] for d in range(2)])      # [2][Bn][4R]
        if s > 0:
            gates = gates + torch.bmm(h[:, :, perm], wt)
        gates = gates.reshape(2, Bn, 4, R)
        cn = torch.sigmoid(gates[:, :, gf]) * c + torch.sigmoid(gates[:, :, gi]) * torch.tanh(gates[:, :, gg])
        hn = torch.sigmoid(gates[:, :, go]) * torch.tanh(cn)
        if h_noise:
            hn = hn * (1.0 + (torch.rand(hn.shape, generator=ng, dtype=F64) * 2 - 1) * h_noise).to(F)
        hn = round16(hn, dtype)
        m = act[None, :, None]
        c = torch.where(m, cn, c)
        h = torch.where(m, hn, h)
        for d in range(2):
            a = rows[act]
            out[a, pos[d][act], d * R:(d + 1) * R] = hn[d][act].to(F64)
    return out, torch.cat([h[0], h[1]], dim=1).to(F64)


def final_from_last_step(out, lens):
    """the final-hidden MUTATION of the host test: [what step T-1 wrote of direction 0 || of direction 1] - right for a full
    sentence (positions T-1 and 0), zeros for a short one, whose last active step came earlier."""
    Bn, T, R2 = out.shape
    full = (torch.as_tensor(lens, dtype=torch.int64) >= T)[:, None]
    z = torch.zeros(Bn, R2 // 2, dtype=out.dtype)
    return torch.cat([torch.where(full, out[:, T - 1, :R2 // 2], z), torch.where(full, out[:, 0, R2 // 2:], z)], dim=1)


def active_mask(lens, T, R):
    """[Bn*T + Bn][2R] bool: the rows the criteria look at (positions below each length, and every final-hidden row)."""
    lens = torch.as_tensor(lens, dtype=torch.int64)
    m = (torch.arange(T)[None, :] < lens[:, None]).reshape(-1)
    return torch.cat([m, torch.ones(len(lens), dtype=torch.bool)])[:, None].expand(-1, 2 * R)


def deviation(got, ref, dtype, mask):
    """-> (largest |got - ref| in ulp, share of elements not bit-equal) over `mask`; all arguments [rows][2R]."""
    d = (got.to(F64) - ref.to(F64)).abs()[mask]
    if not bool(torch.isfinite(d).all()):
        return math.inf, 1.0
    return float(d.max()) / ULP[dtype], float((d != 0).double().mean())


def share_bound(ref_share):
    return SHARE_FACTOR * max(ref_share, SHARE_FLOOR)


def stack_rows(out, fin):
    """out [Bn][T][2R], fin [Bn][2R] -> the kernels' row order [Bn*T + Bn][2R]."""
    return torch.cat([out.reshape(-1, out.shape[-1]), fin])


# ---- inputs ----------------------------------------------------------------------------------------------------------
def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


_W = {}


def rand_whh(R, scale=2.0):
    """[2][4R][R] fp32, uniform in +-scale / sqrt(R) (twice nn.LSTM's init: see the sensitivity condition); one per width."""
    if (R, scale) not in _W:
        g = torch.Generator().manual_seed(seed_of("whh", R))
        _W[(R, scale)] = ((torch.rand(2, 4 * R, R, generator=g) * 2 - 1) * (scale / math.sqrt(R))).contiguous()
    return _W[(R, scale)]


def prepped_whh(R, dtype, acc="f64", zero_slice=False, perm_seed=1):
    """prep_whh of rand_whh(R), cached; zero_slice: with the last 32 columns (one MFMA k-step) zeroed - the sensitivity probe."""
    key = ("prep", R, dtype, acc, zero_slice, perm_seed)
    if key not in _W:
        w = rand_whh(R)
        if zero_slice:
            w = w.clone()
            w[:, :, R - 32:] = 0.0
        _W[key] = prep_whh(w, dtype, acc, perm_seed)
    return _W[key]


def rand_wih(R, K):
    """[2][4R][K] fp32 with unit-variance products against a unit-variance input, and the bias [2][4R]."""
    key = ("wih", R, K)
    if key not in _W:
        g = torch.Generator().manual_seed(seed_of(*key))
        w = ((torch.rand(2, 4 * R, K, generator=g) * 2 - 1) * math.sqrt(3.0 / K)).contiguous()
        _W[key] = (w, (torch.rand(2, 4 * R, generator=g) - 0.5).contiguous())
    return _W[key]


def rand_gx(Bn, T, R, seed):
    """position-indexed gate inputs [2][Bn][T][4R] fp32, O(1)."""
    return torch.randn(2, Bn, T, 4 * R, generator=torch.Generator().manual_seed(seed))


def make_lens(kind, Bn, T):
    """all T / all 1 / a mix that holds both 1 and T (Bn >= 2; lengths in between where there is room)."""
    if kind == "full" or Bn == 1 and kind == "mix":
        return [T] * Bn
    if kind == "ones":
        return [1] * Bn
    assert kind == "mix", kind
    mid = [max(1, (7 * i + 3) % T + 1) for i in range(Bn)]
    mid[0], mid[1] = T, 1
    if Bn > 3:
        mid[-1] = T
    return mid


def project(x, w_ih, bias, dtype):
    """fused form: x [Bn][T][K], w_ih [2][4R][K], bias [2][4R] -> gx [2][Bn][T][4R] float64 from the ROUNDED operands."""
    xr, wr = round16(x.to(F64), dtype), round16(w_ih.to(F64), dtype)
    return torch.einsum("btk,dgk->dbtg", xr, wr) + bias.to(F64)[:, None, None, :]


def make_gxs(gx, lens):
    """[2][T][Bn][4R] fp32 in (direction, STEP) order, as lstm_dev.h indexes it. Rows of inactive steps are NaN: the GEMM
    that fills this tensor in the product never writes them (vog_lstm_schedule gives -1), so no kernel may use them."""
    _, Bn, T, R4 = gx.shape
    gxs = torch.full((2, T, Bn, R4), float("nan"), dtype=torch.float32)
    for b, ln in enumerate(lens):
        for s in range(ln):
            gxs[0, s, b] = gx[0, b, s]
            gxs[1, s, b] = gx[1, b, ln - 1 - s]
    return gxs


def frag_a_index(M, K):
    """halfword index of element (m, k) of an [M][K] matrix in A-fragment order (frag_a, csrc/common.h), [M][K] int64."""
    m, k = np.arange(M, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return ((((m >> 4) * (K >> 5) + (k >> 5)) * 64) + (((k >> 3) & 3) << 4) + (m & 15)) * 8 + (k & 7)


def to_frag_a(x16, pad_bits):
    """[M][K] int16 (16-bit patterns) -> A-fragment order with the last 16-row tile's pad rows allocated and set to
    `pad_bits` (a NaN pattern in the tests: those rows are MFMA columns of their own and must not reach a real column)."""
    M, K = x16.shape
    M16 = (M + 15) // 16 * 16
    full = np.full((M16, K), pad_bits, dtype=np.uint16)
    full[:M] = x16.numpy().view(np.uint16)
    dst = np.empty(M16 * K, dtype=np.uint16)
    dst[frag_a_index(M16, K).reshape(-1)] = full.reshape(-1)
    return torch.from_numpy(dst.view(np.int16))


def from_frag_a(buf16, M, K):
    """the [M][K] int16 view of an A-fragment-ordered buffer (inverse of to_frag_a, without the pad rows)."""
    return torch.from_numpy(buf16.numpy().view(np.uint16)[frag_a_index(M, K)].view(np.int16))


def bits16(x, dtype):
    """float tensor -> int16 patterns of its 16-bit rounding (torch's own conversion)."""
    return x.to(torch.float32).to(T16[dtype]).view(torch.int16)


def pack_w(lib, w, R, K, dtype_code):
    """the library's own vog_lstm_pack_w / vog_lstm_pack_whh (host functions): w [2][4R][K] fp32 -> int16
    [dir][unit/4][K/32][lane][8]."""
    w = w.to(torch.float32).contiguous()
    dst = torch.zeros(2 * 4 * R * K, dtype=torch.int16)
    if K == R:
        rc = lib.vog_lstm_pack_whh(C.c_void_p(w[0].data_ptr()), C.c_void_p(w[1].data_ptr()), C.c_void_p(dst.data_ptr()), R, dtype_code)
    else:
        rc = lib.vog_lstm_pack_w(C.c_void_p(w[0].data_ptr()), C.c_void_p(w[1].data_ptr()), C.c_void_p(dst.data_ptr()), R, K, dtype_code)
    assert rc == 0, rc
    return dst


def make_table(V, R, Bn, T, lens, seed):
    """gate table [V+1][2][R][4] fp32 and tok [Bn*T] int32 -> (table, tok, gx [2][Bn][T][4R]). Active positions draw from
    rows 0 .. V including both ends (position 0 of sentence 0 is row 0, its last one row V); rows V-2 and V-1 hold large
    values and are used only at padded positions, where nothing may read them."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(V + 1, 2, 4 * R, generator=g)
    rows[V - 2:V] = 3.0e4
    tok = torch.randint(0, V - 2, (Bn, T), generator=g, dtype=torch.int64)
    tok[0, 0] = 0
    tok[0, lens[0] - 1] = V if lens[0] > 1 else 0
    if Bn > 1:
        tok[1, 0] = V
    for b, ln in enumerate(lens):
        tok[b, ln:] = V - 2 + (b & 1)
    gx = rows[tok].permute(2, 0, 1, 3).contiguous()                            # [2][Bn][T][4R]
    table = rows.reshape(V + 1, 2, 4, R).permute(0, 1, 3, 2).contiguous()     # [V+1][2][R][4 gates]
    return table, tok.reshape(-1).to(torch.int32), gx


# ---- case families ---------------------------------------------------------------------------------------------------
LAYER_R = (32, 64, 128, 1024)
T_SET = (1, 2, 3, 4, 20)
LENS_KINDS = ("full", "ones", "mix")


def layer_bn(R):
    return (1, 4, 5, 13, 16) if R == 1024 else (1, 5, 16)


def lens_cases(Bn, T):
    """the distinct lens lists of (Bn, T): all T, all 1, a mix holding both."""
    seen, outl = set(), []
    for kind in LENS_KINDS:
        ln = make_lens(kind, Bn, T)
        if tuple(ln) not in seen:
            seen.add(tuple(ln))
            outl.append((kind, ln))
    return outl


def gxs_families():
    """(R, Bn, T, kind, lens) of the `gxs` form's widest sweep."""
    return [(R, Bn, T, kind, ln) for R in LAYER_R for Bn in layer_bn(R) for T in T_SET for kind, ln in lens_cases(Bn, T)]


STEP_R = (32, 96, 1024)
STEP_BN = (1, 16, 17, 33)
STEP_T = 5


def step_families():
    return [(R, Bn, STEP_T, "mix", make_lens("mix", Bn, STEP_T)) for R in STEP_R for Bn in STEP_BN]


FUSED_K = (256, 512, 768, 2048)                         # 1, 2, 3 and 8 chunks of the double-buffered prologue loop
FUSED_R = (32, 128, 1024)
FUSED_SHAPES = ((1, 1), (4, 4), (1, 17), (4, 20), (16, 5))   # Bn*T = 1, 16, 17, 80, 80
TABLE_R = (32, 128, 1024)
TABLE_SHAPES = ((16, 24), (1, 1), (5, 2), (13, 3), (4, 20), (16, 3))
TABLE_V = 40


def fused_families():
    return [(R, Bn, T, "mix", make_lens("mix", Bn, T)) for R in FUSED_R for Bn, T in FUSED_SHAPES]


def table_families():
    return [(R, Bn, T, "mix", make_lens("mix", Bn, T)) for R in TABLE_R for Bn, T in TABLE_SHAPES]


def all_families():
    """every (R, Bn, T, lens) the GPU tests run, once"""
    seen, outl = set(), []
    for f in gxs_families() + step_families() + fused_families() + table_families():
        if (f[0], f[1], f[2], tuple(f[4])) not in seen:
            seen.add((f[0], f[1], f[2], tuple(f[4])))
            outl.append(f)
    return outl


# ---- inputs of a case: drawn until criterion (b) is a stable question ----------------------------------------------------
# A rounding flip of one h early in a sentence changes every later gate of that sentence a little, and some of those land on
# the other side of THEIR rounding boundaries: a cascade. Where the compared population is one or two sentences and the
# reference pair happens to agree (share below the 1 % floor, bound 4 %), a single near-tie decides whether a faithful
# evaluation shows 0.1 % or 5 % of unequal elements (measured: R = 32, Bn = 1, T = 20, f16 - the float64 / float32 pair
# differs on 0.07 %, float32 evaluations with a relative perturbation of 1e-7 ... 1e-6 on 0.1 % or on 4.84 %, always the same
# 65 elements). Such inputs make (b) a coin toss for ANY correct implementation, so they are not used: a draw is kept only
# if it is `settled` - a condition on CPU evaluations alone: faithful evaluations pass (b) on it, whichever side they land.
PROBES, PROBE_NOISE, ROOMY_SHARE, MAX_DRAWS = 6, 2.0 ** -23, 0.02, 12


def settled(gx, R, lens, dtype):
    """-> (ok, r64 rows, reference-pair share, reference-pair deviation in ulp). ok: each of PROBES further float32 evaluations
    (another k permutation, and every h perturbed by up to one float32 ulp, 2^-23 relative, before it is rounded to 16
    bits - the least any float32 evaluation of the gates is away from the exact value; at R = 32 the float32 dot product of
    16-bit operands is all but exact and the permutation alone moves nothing) stays within HALF the (b) bound. Not probed where
    the reference pair itself differs on 2 % or more: the bound is then 8 % or more of a population with many flips, which one
    cascade does not move."""
    T = gx.shape[2]
    mask = active_mask(lens, T, R)
    r64 = stack_rows(*bilstm_ref(gx, prepped_whh(R, dtype), lens, dtype))
    noise, pair = deviation(stack_rows(*bilstm_ref(gx, prepped_whh(R, dtype, "f32perm"), lens, dtype)), r64, dtype, mask)
    if pair >= ROOMY_SHARE or max(lens) < 3:                     # (no cascade without a third step)
        return True, r64, pair, noise
    # (the probes run as one evaluation of PROBES copies of the batch: one pass over the weights per step; they share a k
    # permutation, other than the pair's, and differ by their perturbations)
    Bn = len(lens)
    po, pf = bilstm_ref(gx.repeat(1, PROBES, 1, 1), prepped_whh(R, dtype, "f32perm", perm_seed=2), list(lens) * PROBES, dtype,
                        h_noise=PROBE_NOISE, noise_seed=3)
    for k in range(PROBES):
        probe = stack_rows(po[k * Bn:(k + 1) * Bn], pf[k * Bn:(k + 1) * Bn])
        if deviation(probe, r64, dtype, mask)[1] > share_bound(pair) / 2:
            return False, r64, pair, noise
    return True, r64, pair, noise


_CASES = {}


def settled_case(key, R, lens, dtype, build):
    """build(draw) -> (gx, extras) for draw = 0, 1, ...: the first settled draw, as {gx, extras, r64, pair, noise, draw}; cached
    (one entry) per key"""
    key = (key, dtype)
    if key not in _CASES:
        _CASES.clear()
        for draw in range(MAX_DRAWS):
            gx, extras = build(draw)
            ok, r64, pair, noise = settled(gx, R, lens, dtype)
            if ok:
                _CASES[key] = {"gx": gx, "extras": extras, "r64": r64, "pair": pair, "noise": noise, "draw": draw}
                break
        else:
            raise AssertionError(("no settled draw", key))
    return _CASES[key]


def family_case(R, Bn, T, kind, lens, dtype):
    """the gxs-form inputs of a family: position-indexed gate inputs [2][Bn][T][4R] (the recurrent weights are rand_whh(R))"""
    return settled_case(("gxs", R, Bn, T, kind), R, lens, dtype,
                        lambda draw: (rand_gx(Bn, T, R, seed_of("gx", R, Bn, T, kind, draw)), None))
