"""Operator tests of the inference path's recurrent kernels (csrc/lstm.hip, csrc/lstm_dev.h), one C-ABI entry at a time:
vog_bilstm_layer (gxs form, fused wih form, gate-table form), vog_bilstm_step, vog_lstm_schedule, vog_lstm_out_to_f32.

Reference: tests/lstm_ref.py - the layer restated on the CPU with the kernels' roundings (16-bit W_hh / W_ih / input, h rounded
to 16 bits after every step) and float64 everywhere else. Values are read back as exact 16-bit patterns, recurrent rows and
final-hidden rows alike, and have to meet, against that restatement:
  (a) every element within 2 ulp (ulp = the spacing just below 1.0: 2^-11 f16, 2^-8 bf16): one ulp is a rounding flip, which
      two CPU evaluations of the restatement show between themselves (test_lstm_ref_host.py); one more covers the kernels'
      __expf / v_rcp_f32 putting a second flip on the same element;
  (b) the share of elements not bit-equal to the restatement at most 4 x the share by which the float64 and the
      float32-permuted restatement differ on the same inputs (floor 1 %).
Rows past each length are exactly 0 and everything is finite although the gate inputs of every inactive step are NaN.
The inputs of a case are random draws that lstm_ref.settled accepts - a condition on CPU evaluations alone, which keeps out
draws on which (b) is decided by one near-tie of a one-sentence population (BiLSTM operator tests: the first draws
gave 4.84 % against 4.00 % at R = 32, Bn = 1, T = 20, f16 and 4.27 % against 4.00 % in the fused form at R = 1024, Bn = 1,
T = 17, bf16, with (a) clean; float32 CPU evaluations of the first input give 0.2 % or 4.84 % depending on a 1e-7 perturbation).
Measured worst cases on an MI355X: (a) 1.00 ulp in every form; (b) 3.58 % against 4.00 % (fused form, bf16, R = 1024, Bn = 1, T = 17).

Every device buffer a kernel writes (out16, hx, sync, the fault counter, h / c of the step kernel) lies between two
pattern-filled bands which are checked after the call; after each layer launch sync[2] and the fault counter must be 0."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests import lstm_ref as lr

pytestmark = pytest.mark.gpu
L = importlib.import_module("vognet-pytorch_amd.lib")
DT = {"f16": L.VOG_F16, "bf16": L.VOG_BF16}
NAN16 = {"f16": 0x7e00, "bf16": 0x7fc0}
FRONT, BACK, PATTERN = 4096, 65536, 0xA5
WORST = {}                                       # (form, dtype) -> [largest deviation in ulp, largest share, its bound, case]


# ---- guarded buffers ---------------------------------------------------------------------------------------------------
class Guarded:
    """device buffers, each between a front band of 4096 and a back band of 65536 pattern bytes"""

    def __init__(self):
        self.bufs = []

    def alloc(self, nbytes, fill, name):
        nbytes = int(nbytes)
        assert nbytes > 0, (name, nbytes)
        buf = torch.full((FRONT + nbytes + BACK,), PATTERN, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 256 == 0
        view = buf[FRONT:FRONT + nbytes]
        view.fill_(fill)
        self.bufs.append((name, buf, nbytes))
        return view

    def check(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                 # a device fault: nothing more is started on the GPU in this session
            pytest.exit(f"device error, session ended: {e}", returncode=3)
        for name, buf, nb in self.bufs:
            for band, lo, hi in (("front", 0, FRONT), ("back", FRONT + nb, FRONT + nb + BACK)):
                bad = (buf[lo:hi] != PATTERN).nonzero()
                assert bad.numel() == 0, f"{band} guard band of `{name}` ({nb} bytes) overwritten: first at byte {int(bad[0])} of the band, {bad.numel()} bytes"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_WDEV = {}


def whh_dev(R, dtype):
    key = ("whh", R, dtype)
    if key not in _WDEV:
        _WDEV[key] = lr.pack_w(L.load(), lr.rand_whh(R), R, R, DT[dtype]).cuda()
    return _WDEV[key]


def wih_dev(R, K, dtype):
    key = ("wih", R, K, dtype)
    if key not in _WDEV:
        for k in [k for k in _WDEV if k[0] == "wih" and k != key]:
            del _WDEV[k]                                                     # (33 MB each at R = 1024, K = 2048)
        w, bias = lr.rand_wih(R, K)
        _WDEV[key] = (lr.pack_w(L.load(), w, R, K, DT[dtype]).cuda(), bias.cuda())
    return _WDEV[key]


def rows16(Bn, T):
    return (Bn * T + Bn + 15) // 16 * 16


def read_rows(out16, Bn, T, R, frag, dtype):
    """the guarded out16 view -> ([Bn*T + Bn][2R] float64 of the exact 16-bit values, their int16 patterns); the pad rows of
    the last 16-row tile must still be zero"""
    n, n16 = Bn * T + Bn, rows16(Bn, T)
    raw = out16.view(torch.int16).cpu()
    bits = lr.from_frag_a(raw, n16, 2 * R) if frag else raw.reshape(n16, 2 * R)
    assert not bool(bits[n:].any()), "rows behind the final-hidden rows written"
    bits = bits[:n].contiguous()
    return bits.view(lr.T16[dtype]).double(), bits


class LayerRun:
    """the buffers of one vog_bilstm_layer problem; launch() arms them as the forward's prologue does (hx 0xffff, sync and
    out16 zero) and runs one launch"""

    def __init__(self, Bn, T, R, dtype, frag):
        self.Bn, self.T, self.R, self.dtype, self.frag = Bn, T, R, dtype, frag
        self.g = Guarded()
        lib = L.load()
        self.out16 = self.g.alloc(rows16(Bn, T) * 2 * R * 2, 0, "out16")
        self.hx = self.g.alloc(lib.vog_bilstm_hx_bytes(Bn, T, R), 0xff, "hx")
        self.sync = self.g.alloc(256 * 4, 0, "sync")
        self.fault = self.g.alloc(4, 0, "fault")

    def arm(self):
        self.out16.fill_(0)
        self.hx.fill_(0xff)
        self.sync.fill_(0)

    def args(self, lens, gxs=None, fused=None, table=None, K=0):
        a = L.LstmLayerArgs()
        self.keep = [torch.tensor(lens, dtype=torch.int64).cuda(), whh_dev(self.R, self.dtype)]
        a.lens, a.whh = _p(self.keep[0]), _p(self.keep[1])
        a.hx, a.sync, a.out16, a.fault = _p(self.hx), _p(self.sync), _p(self.out16), _p(self.fault)
        a.Bn, a.T, a.R, a.dtype, a.out_frag, a.inject_stall = self.Bn, self.T, self.R, DT[self.dtype], self.frag, 0
        if gxs is not None:
            self.keep.append(gxs.cuda().contiguous())
            a.gxs = _p(self.keep[-1])
        if fused is not None:
            xa, wih, bias = fused
            self.keep += [xa.cuda(), wih, bias]
            a.xa, a.wih, a.bias, a.K = _p(self.keep[-3]), _p(wih), _p(bias), K
        if table is not None:
            self.keep += [table[0].cuda().contiguous(), table[1].cuda().contiguous()]
            a.gx_table, a.tok = _p(self.keep[-2]), _p(self.keep[-1])
        return a

    def launch(self, a):
        self.arm()
        L.check(L.load().vog_bilstm_layer(C.byref(a), L.stream_ptr()), "vog_bilstm_layer")
        self.g.check()
        sync = self.sync.view(torch.int32).cpu()
        assert int(sync[2]) == 0 and int(self.fault.view(torch.int32)[0]) == 0, \
            f"a hand-off of the layer kernel timed out (sync[2] = {int(sync[2])}, fault counter = {int(self.fault.view(torch.int32)[0])})"
        return read_rows(self.out16, self.Bn, self.T, self.R, self.frag, self.dtype)

    def refused(self, a):
        """the entry returns nonzero and nothing ran: out16 still zero, every hand-off slot still armed"""
        self.arm()
        rc = L.load().vog_bilstm_layer(C.byref(a), L.stream_ptr())
        self.g.check()
        assert rc != 0
        assert not bool(self.out16.any()) and bool((self.hx == 0xff).all()) and not bool(self.sync.any())


def verify(form, case, got, bits, cs, R, lens, T, dtype):
    """the two criteria, zeros past each length, finiteness; prints the measured figures. cs: the case's inputs with their
    float64 restatement and the share by which the float32-permuted one differs from it (lstm_ref.settled_case)"""
    r64, ref_share = cs["r64"], cs["pair"]
    mask = lr.active_mask(lens, T, R)
    assert bool(torch.isfinite(got).all()), (form, case, "not finite")
    assert not bool(bits[~mask].any()), (form, case, "rows past a sentence's length are not exactly 0")
    dev, share = lr.deviation(got, r64, dtype, mask)
    bound = lr.share_bound(ref_share)
    print(f"    {form} {dtype} {case}: {dev:.2f} ulp, unequal {100 * share:.2f} % (reference pair {100 * ref_share:.2f} %, bound {100 * bound:.2f} %)")
    w = WORST.setdefault((form, dtype), [0.0, 0.0, 0.0, ""])
    w[0] = max(w[0], dev)
    if share / bound >= w[1] / max(w[2], 1e-30):
        w[1], w[2], w[3] = share, bound, case
    assert dev <= lr.MAX_ULP, (form, case, dev)
    assert share <= bound, (form, case, share, bound)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (form, dtype), (dev, share, bound, case) in sorted(WORST.items()):
        print(f"\n    WORST {form} {dtype}: (a) {dev:.2f} ulp; (b) {100 * share:.2f} % against a bound of {100 * bound:.2f} % at {case}")


# ---- vog_bilstm_layer, gxs form ----------------------------------------------------------------------------------------
def run_gxs(R, Bn, T, kind, lens, dtype, frag, tag=""):
    cs = lr.family_case(R, Bn, T, kind, lens, dtype)
    run = LayerRun(Bn, T, R, dtype, frag)
    got, bits = run.launch(run.args(lens, gxs=lr.make_gxs(cs["gx"], lens)))
    verify("layer/gxs", f"R={R} Bn={Bn} T={T} lens={kind} frag={frag}{tag}", got, bits, cs, R, lens, T, dtype)
    return bits


RBN = [(R, Bn) for R in lr.LAYER_R for Bn in lr.layer_bn(R)]


@pytest.mark.parametrize("R,Bn", RBN)
def test_layer_gxs_sweep(R, Bn):
    """the widest sweep (f16, fragment-ordered output): T in {1, 2, 3, 4, 20} x lens {all T, all 1, a mix holding both}. The
    small widths may land on either publish flavour (all workgroups of a direction on one XCD or not - decided by placement,
    which the test does not steer): R = 64 and R = 128 run every case twice."""
    for (_, _, T, kind, lens) in [f for f in lr.gxs_families() if f[0] == R and f[1] == Bn]:
        first = run_gxs(R, Bn, T, kind, lens, "f16", 1)
        if R in (64, 128):
            again = run_gxs(R, Bn, T, kind, lens, "f16", 1, " (second run)")
            # (the two publish flavours hand on the same 16-bit values)
            assert torch.equal(first, again), (R, Bn, T, kind)


@pytest.mark.parametrize("dtype,frag", [("f16", 0), ("bf16", 0), ("bf16", 1)])
@pytest.mark.parametrize("R,Bn", RBN)
def test_layer_gxs_dtypes_and_layouts(R, Bn, dtype, frag):
    """the other dtype and the row-major output at every width, Bn and T, ragged lens (all T at Bn = 1)"""
    for T in lr.T_SET:
        run_gxs(R, Bn, T, "mix", lr.make_lens("mix", Bn, T), dtype, frag)
        if R in (64, 128) and T == 20:
            run_gxs(R, Bn, T, "mix", lr.make_lens("mix", Bn, T), dtype, frag, " (second run)")


# ---- vog_bilstm_layer, fused wih form ----------------------------------------------------------------------------------
def fused_case(R, Bn, T, K, lens, dtype):
    w_ih, bias = lr.rand_wih(R, K)
    w64 = lr.round16(w_ih.to(lr.F64), dtype)

    def build(draw):
        x = torch.randn(Bn, T, K, generator=torch.Generator().manual_seed(lr.seed_of("x", R, Bn, T, K, draw)))
        gx = torch.einsum("btk,dgk->dbtg", lr.round16(x.to(lr.F64), dtype), w64) + bias.to(lr.F64)[:, None, None, :]   # lr.project
        return gx, lr.to_frag_a(lr.bits16(x.reshape(Bn * T, K), dtype), NAN16[dtype])

    return lr.settled_case(("fused", R, Bn, T, K), R, lens, dtype, build)


@pytest.mark.parametrize("R,K,dtype", [(R, K, "f16") for R in lr.FUSED_R for K in lr.FUSED_K] + [(R, 768, "bf16") for R in lr.FUSED_R]
                         + [(1024, 2048, "bf16")])
def test_layer_fused(R, K, dtype):
    """x W_ih^T + bias in the kernel's prologue: K / 256 = 1, 2, 3, 8 chunks (single, even, odd), Bn*T = 1, 16, 17, 80 columns
    (the 16-column tile boundary and the maximum); the pad rows of the input's last tile hold NaN"""
    wih, bias = wih_dev(R, K, dtype)
    for Bn, T in lr.FUSED_SHAPES:
        lens = lr.make_lens("mix", Bn, T)
        cs = fused_case(R, Bn, T, K, lens, dtype)
        run = LayerRun(Bn, T, R, dtype, 1)
        got, bits = run.launch(run.args(lens, fused=(cs["extras"], wih, bias), K=K))
        verify("layer/fused", f"R={R} K={K} Bn={Bn} T={T}", got, bits, cs, R, lens, T, dtype)


# ---- vog_bilstm_layer, gate-table form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R", lr.TABLE_R)
def test_layer_table(R, dtype):
    """gate inputs from the per-token table: up to the 384 staged token ids (Bn = 16, T = 24), T = 1, 2, 3 where the
    three-step preload runs past the sequence, ragged lens; padded positions name rows of large values"""
    for Bn, T in lr.TABLE_SHAPES:
        lens = lr.make_lens("mix", Bn, T)
        def build(draw):
            table, tok, gx = lr.make_table(lr.TABLE_V, R, Bn, T, lens, lr.seed_of("tab", R, Bn, T, draw))
            return gx, (table, tok)

        cs = lr.settled_case(("table", R, Bn, T), R, lens, dtype, build)
        run = LayerRun(Bn, T, R, dtype, 1)
        got, bits = run.launch(run.args(lens, table=cs["extras"]))
        verify("layer/table", f"R={R} Bn={Bn} T={T}", got, bits, cs, R, lens, T, dtype)


# ---- vog_bilstm_layer: re-use, refusals --------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [32, 1024])
def test_layer_reuse_of_buffers(R):
    """a second launch on the same buffers after re-arming, with other lens and data, equals a fresh-buffer run bit for bit"""
    Bn, T = 5, 7
    lens1, lens2 = [7, 1, 4, 7, 2], [2, 7, 7, 1, 5]
    gx1 = lr.rand_gx(Bn, T, R, 11)
    cs = lr.settled_case(("reuse", R), R, lens2, "f16", lambda draw: (lr.rand_gx(Bn, T, R, 12 + draw), None))
    gx2 = cs["gx"]
    run = LayerRun(Bn, T, R, "f16", 1)
    run.launch(run.args(lens1, gxs=lr.make_gxs(gx1, lens1)))
    got, bits = run.launch(run.args(lens2, gxs=lr.make_gxs(gx2, lens2)))
    fresh = LayerRun(Bn, T, R, "f16", 1)
    _, bits_fresh = fresh.launch(fresh.args(lens2, gxs=lr.make_gxs(gx2, lens2)))
    assert torch.equal(bits, bits_fresh)
    verify("layer/gxs", f"R={R} Bn={Bn} T={T} re-used buffers", got, bits, cs, R, lens2, T, "f16")


def test_layer_refusals():
    R = 32
    # fused form: 81 columns, K = 128
    for Bn, T, K in ((1, 81, 256), (4, 4, 128)):
        w_ih, bias = lr.rand_wih(R, 256)
        run = LayerRun(Bn, T, R, "f16", 1)
        xa = torch.zeros((Bn * T + 15) // 16 * 16 * 256, dtype=torch.int16)
        run.refused(run.args([T] * Bn, fused=(xa, lr.pack_w(L.load(), w_ih, R, 256, DT["f16"]).cuda(), bias.cuda()), K=K))
    # gate table: 385 token ids
    Bn, T = 1, 385
    table, tok, _ = lr.make_table(lr.TABLE_V, R, Bn, T, [T], 3)
    run = LayerRun(Bn, T, R, "f16", 1)
    run.refused(run.args([T], table=(table, tok)))
    a = run.args([T], table=(table, tok))
    a.tok = None
    run.refused(a)
    # no input form at all, T = 0
    run = LayerRun(2, 3, R, "f16", 1)
    run.refused(run.args([3, 1]))
    a = run.args([3, 1], gxs=lr.make_gxs(lr.rand_gx(2, 3, R, 1), [3, 1]))
    a.T = 0
    run.refused(a)


def test_layer_supported_agrees_with_entry():
    """vog_bilstm_layer_supported and what the entry accepts, Bn 0 .. 17 x R in {0, 16, 32, 64, 96, 128, 256, 1024, 2080}"""
    lib = L.load()
    T = 2
    for R in (0, 16, 32, 64, 96, 128, 256, 1024, 2080):
        for Bn in range(18):
            want = bool(lib.vog_bilstm_layer_supported(Bn, R))
            assert want == (1 <= Bn <= 16 and R in (32, 64, 128, 1024)), (Bn, R)
            if want:
                run_gxs(R, Bn, T, "mix", lr.make_lens("mix", Bn, T), "f16", 1, " (supported sweep)")
            else:
                # buffers of a shape that is supported and at least as large; only the refused (Bn, R) go into the arguments
                run = LayerRun(max(Bn, 1), T, 32 * max(1, -(-R // 32)), "f16", 1)
                run.R = 32                                                   # (which weights: any)
                a = run.args([T] * max(Bn, 1), gxs=torch.zeros(2, T, max(Bn, 1), 4 * max(R, 32)))
                a.Bn, a.R = Bn, R
                run.refused(a)


# ---- vog_bilstm_step ---------------------------------------------------------------------------------------------------
def run_steps(R, Bn, T, lens, gx, dtype, frag):
    lib = L.load()
    g = Guarded()
    Bn16 = (Bn + 15) // 16 * 16
    n16 = rows16(Bn, T)
    out16 = g.alloc(n16 * 2 * R * 2, 0, "out16")
    h = [g.alloc(Bn16 * 2 * R * 2, 0, f"h{i}") for i in range(2)]
    c = g.alloc(Bn16 * 2 * R * 4, 0, "c")
    gxs, lens_d, whh = lr.make_gxs(gx, lens).cuda(), torch.tensor(lens, dtype=torch.int64).cuda(), whh_dev(R, dtype)
    a = L.LstmStepArgs()
    a.gx, a.whh, a.c, a.out16, a.lens = _p(gxs), _p(whh), _p(c), _p(out16), _p(lens_d)
    a.Bn, a.T, a.R, a.dtype, a.out_frag, a.final_row0 = Bn, T, R, DT[dtype], frag, Bn * T
    for s in range(T):
        a.step, a.h_in, a.h_out = s, _p(h[s & 1]), _p(h[(s + 1) & 1])
        L.check(lib.vog_bilstm_step(C.byref(a), L.stream_ptr()), "vog_bilstm_step")
    g.check()
    last = h[T & 1].view(torch.int16).cpu().reshape(Bn16, 2 * R)
    assert not bool(last[Bn:].any()), "state rows past Bn written"
    if frag:
        got, bits = read_rows(out16, Bn, T, R, 1, dtype)
        # the state the last step left is the final hidden state too
        assert torch.equal(bits[Bn * T:], last[:Bn])
    else:
        # row-major: [Bn*T][2R] only; the final hidden state is the state the last step left
        raw = out16.view(torch.int16).cpu().reshape(n16, 2 * R)
        assert not bool(raw[Bn * T:].any()), "rows behind the Bn*T output rows written"
        bits = torch.cat([raw[:Bn * T], last[:Bn]]).contiguous()
        got = bits.view(lr.T16[dtype]).double()
    # h_in == h_out is refused, nothing runs
    before = [t.clone() for t in (out16, h[0], h[1], c)]
    a.step, a.h_in, a.h_out = 0, _p(h[0]), _p(h[0])
    assert lib.vog_bilstm_step(C.byref(a), L.stream_ptr()) != 0
    g.check()
    assert all(torch.equal(x, y) for x, y in zip(before, (out16, h[0], h[1], c)))
    return got, bits


@pytest.mark.parametrize("frag", [0, 1])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R,Bn", [(R, Bn) for R in lr.STEP_R for Bn in lr.STEP_BN])
def test_step(R, Bn, dtype, frag):
    """T launches on ping-pong h (rows padded to 16) and c: R = 96 lies outside the persistent set, Bn = 17 / 33 leave a
    partial second / third batch tile"""
    T, lens = lr.STEP_T, lr.make_lens("mix", Bn, lr.STEP_T)
    cs = lr.family_case(R, Bn, T, "mix", lens, dtype)
    got, bits = run_steps(R, Bn, T, lens, cs["gx"], dtype, frag)
    verify("step", f"R={R} Bn={Bn} T={T} frag={frag}", got, bits, cs, R, lens, T, dtype)


# ---- small entries: exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,T", [(1, 1), (1, 20), (5, 1), (5, 20)])
def test_schedule(Bn, T):
    """rows[dir*Bn*T + b*T + t] = dir*(T*Bn - 1) + step*Bn + b with step = t (dir 0) or len_b-1-t (dir 1); -1 for t >= len_b"""
    for lens in (lr.make_lens("mix", Bn, T), lr.make_lens("ones", Bn, T), [max(1, T - 3 * b) for b in range(Bn)]):
        g = Guarded()
        rows = g.alloc(2 * Bn * T * 4, 0x5a, "rows")
        lens_d = torch.tensor(lens, dtype=torch.int64).cuda()
        L.check(L.load().vog_lstm_schedule(_p(lens_d), _p(rows), Bn, T, L.stream_ptr()), "vog_lstm_schedule")
        g.check()
        want = np.empty((2, Bn, T), dtype=np.int32)
        for b in range(Bn):
            for t in range(T):
                want[0, b, t] = t * Bn + b if t < lens[b] else -1
                want[1, b, t] = (T * Bn - 1) + (lens[b] - 1 - t) * Bn + b if t < lens[b] else -1
        assert np.array_equal(rows.view(torch.int32).cpu().numpy().reshape(2, Bn, T), want), (Bn, T, lens)


@pytest.mark.parametrize("frag", [0, 1])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_out_to_f32(dtype, frag):
    rows_x, rows_f, W = 21, 3, 64
    g = Guarded()
    bits = torch.randint(-32768, 32767, (rows_x + rows_f, W), generator=torch.Generator().manual_seed(7), dtype=torch.int16)
    expo = 0x7c00 if dtype == "f16" else 0x7f80
    bits[(bits & expo) == expo] = 0x0001                                   # no h is infinite or NaN; a subnormal instead
    src = lr.to_frag_a(bits, 0) if frag else bits.reshape(-1)
    x = g.alloc(rows_x * W * 4, 0x5a, "x")
    fin = g.alloc(rows_f * W * 4, 0x5a, "fin")
    src_d = src.cuda()
    L.check(L.load().vog_lstm_out_to_f32(_p(src_d), frag, rows_x, rows_f, W, DT[dtype], _p(x), _p(fin), L.stream_ptr()), "vog_lstm_out_to_f32")
    g.check()
    want = bits.view(lr.T16[dtype]).float().view(torch.int32)              # widened: bit patterns, NaNs included
    gotb = torch.cat([x.view(torch.int32).cpu().reshape(rows_x, W), fin.view(torch.int32).cpu().reshape(rows_f, W)])
    assert torch.equal(gotb, want)
