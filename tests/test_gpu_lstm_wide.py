"""Operator tests of the wide persistent BiLSTM layer kernel (vog_bilstm_layer_wide: 17 .. 32 sentences, csrc/lstm_dev.h
LstmLayerWideBody), one C-ABI entry at a time.

1. Bit equality with the narrow kernel. A lane of the wide kernel carries sentence b and sentence b + 16 with the arithmetic
   of the narrow kernel, and sentences never interact: one wide launch must return the BITS of two vog_bilstm_layer launches
   over sentences [0, 16) and [16, Bn) on the same inputs sliced per half (own hx / sync), recurrent rows and final-hidden
   rows alike, in both out16 layouts. No tolerance.
2. Criteria (a) and (b) of tests/test_gpu_lstm_ops.py against the float64 restatement of tests/lstm_ref.py (2 ulp; share of
   unequal elements at most 4 x the restatement pair's, floor 1 %) at Bn = 32; tests/test_lstm_wide_host.py holds the
   conditions on the restatement alone for these shapes.
3. Every buffer a launch writes (out16, hx, sync, the fault counter) lies between two pattern-filled bands which are checked
   after every call; after every launch sync[2] == 0 and the fault counter is unchanged.
4. Refusals. 5. The poison contract with the immediate test hook (inject_stall = 1: no real wait anywhere).

Inactive gate inputs are NaN and padded table positions name rows of 3e4, as in test_gpu_lstm_ops.py."""
import ctypes as C
import importlib

import pytest
import torch

from tests import lstm_ref as lr
from tests.test_lstm_wide_host import WIDE_CRIT          # the shapes whose restatement pair the host test holds to the bounds

pytestmark = pytest.mark.gpu
L = importlib.import_module("vognet-pytorch_amd.lib")
DT = {"f16": L.VOG_F16, "bf16": L.VOG_BF16}
FRONT, BACK, PATTERN = 4096, 65536, 0xA5
WIDE, NARROW = "vog_bilstm_layer_wide", "vog_bilstm_layer"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Guarded:
    """device buffers, each between a front band of 4096 and a back band of 65536 pattern bytes"""

    def __init__(self):
        self.bufs = []

    def alloc(self, nbytes, fill, name):
        nbytes = int(nbytes)
        assert nbytes > 0, (name, nbytes)
        buf = torch.full((FRONT + nbytes + BACK,), PATTERN, dtype=torch.uint8, device="cuda")
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


_WDEV = {}


def whh_dev(R, dtype):
    if (R, dtype) not in _WDEV:
        _WDEV[(R, dtype)] = lr.pack_w(L.load(), lr.rand_whh(R), R, R, DT[dtype]).cuda()
    return _WDEV[(R, dtype)]


def rows16(Bn, T):
    return (Bn * T + Bn + 15) // 16 * 16


class Run:
    """the guarded buffers of one layer problem (sized for `Bn` sentences) and launches of either entry on them"""

    def __init__(self, Bn, T, R, dtype, frag):
        self.Bn, self.T, self.R, self.dtype, self.frag = Bn, T, R, dtype, frag
        self.g = Guarded()
        self.out16 = self.g.alloc(rows16(Bn, T) * 2 * R * 2, 0, "out16")
        self.hx = self.g.alloc(L.load().vog_bilstm_hx_bytes(Bn, T, R), 0xff, "hx")
        self.sync = self.g.alloc(256 * 4, 0, "sync")
        self.fault = self.g.alloc(4, 0, "fault")

    def args(self, lens, gxs=None, table=None):
        a = L.LstmLayerArgs()
        self.keep = [torch.tensor(lens, dtype=torch.int64).cuda(), whh_dev(self.R, self.dtype)]
        a.lens, a.whh = _p(self.keep[0]), _p(self.keep[1])
        a.hx, a.sync, a.out16, a.fault = _p(self.hx), _p(self.sync), _p(self.out16), _p(self.fault)
        a.Bn, a.T, a.R, a.dtype, a.out_frag, a.inject_stall = self.Bn, self.T, self.R, DT[self.dtype], self.frag, 0
        if gxs is not None:
            self.keep.append(gxs.cuda().contiguous())
            a.gxs = _p(self.keep[-1])
        if table is not None:
            self.keep += [table[0].cuda().contiguous(), table[1].cuda().contiguous()]
            a.gx_table, a.tok = _p(self.keep[-2]), _p(self.keep[-1])
        return a

    def arm(self):
        self.out16.fill_(0)
        self.hx.fill_(0xff)
        self.sync.fill_(0)

    def bits(self):
        """out16 -> [Bn*T + Bn][2R] int16 patterns; the pad rows of the last 16-row tile must still be zero"""
        n, n16 = self.Bn * self.T + self.Bn, rows16(self.Bn, self.T)
        raw = self.out16.view(torch.int16).cpu()
        b = lr.from_frag_a(raw, n16, 2 * self.R) if self.frag else raw.reshape(n16, 2 * self.R)
        assert not bool(b[n:].any()), "rows behind the final-hidden rows written"
        return b[:n].contiguous()

    def launch(self, a, entry=WIDE, stalled=False):
        self.arm()
        fault0 = int(self.fault.view(torch.int32)[0])
        L.check(getattr(L.load(), entry)(C.byref(a), L.stream_ptr()), entry)
        self.g.check()
        sync2, fault = int(self.sync.view(torch.int32)[2]), int(self.fault.view(torch.int32)[0])
        if stalled:
            assert sync2 != 0, "a stalled launch leaves sync[2] set"
            assert fault == fault0 + 1, (fault0, fault)
        else:
            assert sync2 == 0 and fault == fault0, f"a hand-off timed out (sync[2] = {sync2}, fault counter {fault0} -> {fault})"
        return self.bits()

    def refused(self, a, entry=WIDE):
        """the entry returns nonzero and nothing ran: out16 still zero, every hand-off slot still armed"""
        self.arm()
        rc = getattr(L.load(), entry)(C.byref(a), L.stream_ptr())
        self.g.check()
        assert rc != 0, entry
        assert not bool(self.out16.any()) and bool((self.hx == 0xff).all()) and not bool(self.sync.any())
        assert int(self.fault.view(torch.int32)[0]) == 0


def wide_lens(Bn, T, variant=0):
    """ragged lengths with 1 and T in BOTH column tiles (sentences [0, 16) and [16, Bn)); at Bn = 17 the second tile has one
    sentence: length T (variant 0) or 1 (variant 1)"""
    lens = lr.make_lens("mix", Bn, T)            # lens[0] = T, lens[1] = 1, lens[-1] = T
    lens[16] = T
    if Bn > 17:
        lens[17] = 1
    elif variant:
        lens[16] = 1
    assert {1, T} <= set(lens[:16]) and (Bn == 17 or {1, T} <= set(lens[16:]))
    return lens


def halves_equal(wide, lo, hi, Bn, T, what):
    """[Bn*T + Bn] rows of the wide launch against the rows of the two narrow launches"""
    n1 = 16
    assert torch.equal(wide[:n1 * T], lo[:n1 * T]), (what, "recurrent rows of sentences [0, 16)")
    assert torch.equal(wide[n1 * T:Bn * T], hi[:(Bn - n1) * T]), (what, "recurrent rows of sentences [16, Bn)")
    assert torch.equal(wide[Bn * T:Bn * T + n1], lo[n1 * T:]), (what, "final-hidden rows of sentences [0, 16)")
    assert torch.equal(wide[Bn * T + n1:], hi[(Bn - n1) * T:]), (what, "final-hidden rows of sentences [16, Bn)")
    assert bool(wide.any()), what


# ---- 1. bit equality with two narrow launches --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R", [32, 128, 1024])
def test_wide_equals_two_narrow_launches_gxs(R, dtype):
    """R = 32: one workgroup per direction (the same-XCD store path); R = 128: four; R = 1024: the full kernel. Bn = 17 leaves
    one live column in the second tile. T = 1 has no hand-off at all."""
    for Bn in (17, 24, 32):
        for T in (1, 5, 20):
            for variant in ((0, 1) if Bn == 17 and T > 1 else (0,)):
                lens = wide_lens(Bn, T, variant)
                gxs = lr.make_gxs(lr.rand_gx(Bn, T, R, lr.seed_of("wide", R, Bn, T)), lens)        # [2][T][Bn][4R], NaN where inactive
                for frag in (1, 0):
                    what = (R, dtype, Bn, T, variant, frag)
                    w = Run(Bn, T, R, dtype, frag)
                    wide = w.launch(w.args(lens, gxs=gxs))
                    lo_run, hi_run = Run(16, T, R, dtype, frag), Run(Bn - 16, T, R, dtype, frag)
                    lo = lo_run.launch(lo_run.args(lens[:16], gxs=gxs[:, :, :16]), NARROW)
                    hi = hi_run.launch(hi_run.args(lens[16:], gxs=gxs[:, :, 16:]), NARROW)
                    halves_equal(wide, lo, hi, Bn, T, what)
                    # rows past each length are exactly 0, everything else finite
                    mask = lr.active_mask(lens, T, R)
                    assert not bool(wide[~mask].any()), what
                    assert bool(torch.isfinite(wide.view(lr.T16[dtype]).float()).all()), what


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R", [32, 128, 1024])
def test_wide_equals_two_narrow_launches_table(R, dtype):
    """the gate-table form at T = 24, Bn = 32 - exactly the 768 token ids the kernel stages - and at shapes where the preload
    runs past the sequence (T = 1, 2) or the second tile is partial"""
    for Bn, T in ((32, 24), (17, 1), (24, 2), (21, 7)):
        lens = wide_lens(Bn, T)
        table, tok, _ = lr.make_table(lr.TABLE_V, R, Bn, T, lens, lr.seed_of("widetab", R, Bn, T))
        tk = tok.reshape(Bn, T)
        for frag in (1, 0):
            w = Run(Bn, T, R, dtype, frag)
            wide = w.launch(w.args(lens, table=(table, tok)))
            lo_run, hi_run = Run(16, T, R, dtype, frag), Run(Bn - 16, T, R, dtype, frag)
            lo = lo_run.launch(lo_run.args(lens[:16], table=(table, tk[:16].reshape(-1))), NARROW)
            hi = hi_run.launch(hi_run.args(lens[16:], table=(table, tk[16:].reshape(-1))), NARROW)
            halves_equal(wide, lo, hi, Bn, T, (R, dtype, Bn, T, frag, "table"))
            assert bool(torch.isfinite(wide.view(lr.T16[dtype]).float()).all())


def test_wide_reuse_of_buffers():
    """a second launch on the same buffers after re-arming, with other lens and data, equals a fresh-buffer run bit for bit"""
    R, Bn, T = 128, 19, 6
    lens1, lens2 = wide_lens(Bn, T), list(reversed(wide_lens(Bn, T)))
    g1, g2 = (lr.make_gxs(lr.rand_gx(Bn, T, R, 70 + i), ln) for i, ln in enumerate((lens1, lens2)))
    run = Run(Bn, T, R, "f16", 1)
    run.launch(run.args(lens1, gxs=g1))
    again = run.launch(run.args(lens2, gxs=g2))
    fresh = Run(Bn, T, R, "f16", 1)
    assert torch.equal(again, fresh.launch(fresh.args(lens2, gxs=g2)))


# ---- 2. criteria (a) and (b) against the float64 restatement -----------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R,Bn,T", WIDE_CRIT)
def test_wide_against_restatement(R, Bn, T, dtype):
    """Measured on an MI355X: (a) 1.00 ulp at most (0.50 at R = 128, bf16); (b) R = 1024 f16 4.27 % against a bound of
    16.98 % (restatement pair 4.25 %), R = 1024 bf16 0.99 % against 4.00 %, R = 128 f16 0.57 % and bf16 0.09 % against 4.00 %."""
    lens = lr.make_lens("mix", Bn, T)
    cs = lr.family_case(R, Bn, T, "mix", lens, dtype)        # inputs chosen by lstm_ref.settled: CPU evaluations alone
    run = Run(Bn, T, R, dtype, 1)
    bits = run.launch(run.args(lens, gxs=lr.make_gxs(cs["gx"], lens)))
    got = bits.view(lr.T16[dtype]).double()
    mask = lr.active_mask(lens, T, R)
    assert bool(torch.isfinite(got).all())
    assert not bool(bits[~mask].any()), "rows past a sentence's length are not exactly 0"
    dev, share = lr.deviation(got, cs["r64"], dtype, mask)
    bound = lr.share_bound(cs["pair"])
    print(f"    wide/gxs {dtype} R={R} Bn={Bn} T={T}: {dev:.2f} ulp, unequal {100 * share:.2f} % "
          f"(reference pair {100 * cs['pair']:.2f} %, bound {100 * bound:.2f} %)")
    assert dev <= lr.MAX_ULP, (R, dtype, dev)
    assert share <= bound, (R, dtype, share, bound)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_wide_refusals():
    R, T = 32, 3
    run = Run(33, T, 128, "f16", 1)                          # buffers at least as large as anything named below
    run.R = R

    def base(Bn):
        a = run.args([T] * max(Bn, 1), gxs=torch.zeros(2, T, max(Bn, 1), 4 * 128))
        a.Bn = Bn
        return a

    for Bn in (0, 16, 33):
        run.refused(base(Bn))
    a = base(20)
    a.R = 96
    run.refused(a)
    a = base(20)
    a.T = 0
    run.refused(a)
    a = base(20)                                             # the in-kernel projection is narrow-only: any wih is refused
    w_ih, bias = lr.rand_wih(R, 256)
    keep = [lr.pack_w(L.load(), w_ih, R, 256, DT["f16"]).cuda(), bias.cuda(), torch.zeros(64 * 256, dtype=torch.int16).cuda()]
    a.wih, a.bias, a.xa, a.K = _p(keep[0]), _p(keep[1]), _p(keep[2]), 256
    run.refused(a)
    a = base(20)                                             # no input form at all
    a.gxs = None
    run.refused(a)
    # gate table: 769 token ids (Bn x T = 769 has no divisor in 17 .. 32; 17 x 46 = 782 is the nearest shape above 768)
    Bn, T2 = 17, 46
    table, tok, _ = lr.make_table(lr.TABLE_V, R, Bn, T2, [T2] * Bn, 3)
    big = Run(Bn, T2, R, "f16", 1)
    big.refused(big.args([T2] * Bn, table=(table, tok)))
    a = big.args([T2] * Bn, table=(table, tok))
    a.T = 45                                                 # 765 ids: accepted by the size rule, refused without tok
    a.tok = None
    big.refused(a)
    # the narrow entry still refuses 17 sentences
    nar = Run(17, T, R, "f16", 1)
    nar.refused(nar.args([T] * 17, gxs=torch.zeros(2, T, 17, 4 * R)), NARROW)


def test_wide_supported_agrees_with_entry():
    lib = L.load()
    T = 2
    for R in (32, 96, 128):
        for Bn in (16, 17, 32, 33):
            want = bool(lib.vog_bilstm_layer_wide_supported(Bn, R))
            assert want == (17 <= Bn <= 32 and R in (32, 128)), (Bn, R)
            if want:
                lens = lr.make_lens("mix", Bn, T)
                run = Run(Bn, T, R, "f16", 1)
                run.launch(run.args(lens, gxs=lr.make_gxs(lr.rand_gx(Bn, T, R, 5), lens)))


# ---- 5. the poison contract, with the immediate hook -------------------------------------------------------------------------
def test_wide_poison_contract():
    """inject_stall = 1: every workgroup behaves as if its first wait had timed out - no wait happens. Every output row is
    NaN, the fault counter is +1; a clean launch on the same buffers afterwards is clean again."""
    Bn, T, R = 32, 5, 128
    lens = wide_lens(Bn, T)
    gxs = lr.make_gxs(lr.rand_gx(Bn, T, R, 9), lens)
    for frag in (1, 0):
        run = Run(Bn, T, R, "f16", frag)
        a = run.args(lens, gxs=gxs)
        a.inject_stall = 1
        bits = run.launch(a, stalled=True)
        assert bool((bits == 0x7fff).all()), "a stalled launch must poison every output row"
        assert bool(torch.isnan(bits.view(torch.float16).float()).all())
        assert int(run.sync.view(torch.int32)[3]) == 1            # (the once-per-launch report word)
        a.inject_stall = 0
        run.fault.fill_(0)
        clean = run.launch(a)
        assert bool(torch.isfinite(clean.view(torch.float16).float()).all())
