"""Host half of the BiLSTM operator tests: the weight packers (host functions of the library), the reference of
tests/lstm_ref.py against torch.nn.LSTM, and the two conditions the reference alone has to meet for every case family that
tests/test_gpu_lstm_ops.py runs - so that the bounds used there (2 ulp; 4 x the reference pair's share of unequal elements)
are neither tighter than two faithful evaluations differ (noise) nor looser than a kernel bug moves the result (sensitivity).
ulp = the spacing just below 1.0: 2^-11 for f16, 2^-8 for bf16."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests import lstm_ref as lr

L = importlib.import_module("vognet-pytorch_amd.lib")
DT = {"f16": L.VOG_F16, "bf16": L.VOG_BF16}


# ---- vog_lstm_pack_w / vog_lstm_pack_whh -----------------------------------------------------------------------------
def _specials(dtype):
    """values whose 16-bit rounding is decided by the tie rule, the subnormal range or the sign of zero"""
    e = 2.0 ** -11 if dtype == "f16" else 2.0 ** -8            # half an ulp of [1, 2)
    v = [0.0, -0.0, 1.0 + e, 1.0 + 3 * e, -(1.0 + e), -(1.0 + 3 * e), 1.0 + e + 2.0 ** -20, 1.0 + e - 2.0 ** -20,
         2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 5 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1e-40, -1e-40,
         2.0 ** -126, 2.0 ** -127, 3 * 2.0 ** -134, 2.0 ** -133 + 2.0 ** -134, 65504.0, 65519.0, 0.1, -0.3]
    return torch.tensor(v, dtype=torch.float32)


def _expected_pack(w, R, K, dtype):
    """[dir][unit/4][K/32][lane][8] from the documented formula: lane = kq * 16 + rr holds, of tile (4 units x 4 gates), row
    rr = unit_local * 4 + gate - i.e. row gate * R + tile * 4 + unit_local of the [4R][K] matrix - and columns
    ks * 32 + kq * 8 + (0 .. 7)."""
    bits = lr.bits16(w, dtype).numpy()                       # [2][4R][K]
    d, tile, ks, lane, j = np.meshgrid(np.arange(2), np.arange(R // 4), np.arange(K // 32), np.arange(64), np.arange(8), indexing="ij")
    rr, kq = lane % 16, lane // 16
    row = (rr % 4) * R + tile * 4 + rr // 4
    col = ks * 32 + kq * 8 + j
    return bits[d, row, col].reshape(-1)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R", [4, 32, 64])
@pytest.mark.parametrize("K", [32, 96, 256])
def test_pack_w_layout_and_rounding(R, K, dtype):
    lib = L.load()
    g = torch.Generator().manual_seed(lr.seed_of("pack", R, K))
    w = torch.randn(2, 4 * R, K, generator=g)
    sp = _specials(dtype)
    w.view(-1)[:len(sp)] = sp                                # direction 0
    w[1].view(-1)[7:7 + len(sp)] = sp                        # direction 1, other lanes
    got = lr.pack_w(lib, w, R, K, DT[dtype]).numpy()
    want = _expected_pack(w, R, K, dtype)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R", [32, 64])
def test_pack_whh_is_pack_w_at_k_equal_r(R, dtype):
    lib = L.load()
    w = lr.rand_whh(R).clone()
    sp = _specials(dtype)
    w.view(-1)[3:3 + len(sp)] = sp
    got = lr.pack_w(lib, w, R, R, DT[dtype]).numpy()          # K == R: goes through vog_lstm_pack_whh
    assert np.array_equal(got, _expected_pack(w, R, R, dtype))


def test_pack_refuses_bad_shapes():
    lib = L.load()
    w = torch.zeros(2, 16, 48)
    dst = torch.zeros(2 * 16 * 48, dtype=torch.int16)
    p = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    assert lib.vog_lstm_pack_w(p(w[0]), p(w[1]), p(dst), 4, 48, L.VOG_F16) != 0        # K % 32
    assert lib.vog_lstm_pack_w(p(w[0]), p(w[1]), p(dst), 6, 32, L.VOG_F16) != 0        # R % 4
    assert lib.vog_lstm_pack_whh(p(w[0]), p(w[1]), p(dst), 4, L.VOG_F16) != 0          # K = R = 4
    assert lib.vog_lstm_pack_w(None, p(w[1]), p(dst), 4, 32, L.VOG_F16) != 0
    assert not dst.any()


# ---- the reference against torch.nn.LSTM -----------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,T,K,R,lens", [(5, 7, 12, 8, [7, 1, 3, 7, 5]), (1, 1, 4, 4, [1]), (3, 4, 6, 32, [2, 4, 1])])
def test_reference_matches_nn_lstm(Bn, T, K, R, lens):
    torch.manual_seed(Bn * 100 + T)
    m = torch.nn.LSTM(K, R, num_layers=1, batch_first=True, bidirectional=True).double()
    x = torch.randn(Bn, T, K, dtype=torch.float64)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(3.0)                                       # gates well away from the linear range
        pk = torch.nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False)
        o, (hn, _) = m(pk)
        want, _ = torch.nn.utils.rnn.pad_packed_sequence(o, batch_first=True, total_length=T)
        w_ih = torch.stack([m.weight_ih_l0, m.weight_ih_l0_reverse])
        w_hh = torch.stack([m.weight_hh_l0, m.weight_hh_l0_reverse])
        bias = torch.stack([m.bias_ih_l0 + m.bias_hh_l0, m.bias_ih_l0_reverse + m.bias_hh_l0_reverse])
        gx = lr.project(x, w_ih, bias, None)
        out, fin = lr.bilstm_ref(gx, w_hh, lens, None)
    assert float((out - want).abs().max()) <= 1e-12
    assert float((fin - torch.cat([hn[0], hn[1]], dim=1)).abs().max()) <= 1e-12
    # the step-ordered form of the same gates: active rows land where lstm_dev.h reads them, the others are NaN
    gxs = lr.make_gxs(gx.float(), lens)
    for b, ln in enumerate(lens):
        assert torch.equal(gxs[0, :ln, b], gx[0, b, :ln].float()) and torch.equal(gxs[1, :ln, b], gx[1, b, :ln].flip(0).float())
        assert bool(torch.isnan(gxs[:, ln:, b]).all())


def test_frag_a_round_trip():
    x = torch.arange(17 * 64, dtype=torch.int16).reshape(17, 64)
    buf = lr.to_frag_a(x, 0x7e00)
    assert buf.numel() == 32 * 64
    assert torch.equal(lr.from_frag_a(buf, 17, 64), x)
    assert int((buf == 0x7e00).sum()) == 15 * 64
    # element (m, k) -> [m/16][K/32][lane = ((k%32)/8)*16 + m%16][k%8] (include/vog_hip.h)
    m, k = 16, 41
    assert int(buf[((m // 16 * 2 + k // 32) * 64 + ((k % 32) // 8) * 16 + m % 16) * 8 + k % 8]) == int(x[m, k])


def test_table_form_inputs():
    lens = [4, 1, 2]
    table, tok, gx = lr.make_table(40, 8, 3, 4, lens, 5)
    tk = tok.reshape(3, 4).long()
    assert int(tk[0, 0]) == 0 and int(tk[0, 3]) == 40 and int(tk[1, 0]) == 40
    for b, ln in enumerate(lens):
        assert bool((tk[b, ln:] >= 38).all()) and bool((tk[b, :ln] < 38).logical_or(tk[b, :ln] == 40).all())
        for t in range(ln):
            for d in range(2):
                assert torch.equal(table[tk[b, t], d].t().reshape(-1), gx[d, b, t])          # [R][4] -> gate-major 4R
    assert float(table[38:40].min()) == 3.0e4


# ---- the two conditions on the reference alone -----------------------------------------------------------------------
def _families(R):
    return [f for f in lr.all_families() if f[0] == R]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R,Bn", sorted({(f[0], f[1]) for f in lr.all_families()}))
def test_reference_noise_and_sensitivity(R, Bn, dtype):
    """Noise: float64 against float32-permuted differ by at most 1 ulp anywhere. Sensitivity: zeroing one 32-column slice of
    W_hh (one MFMA k-step) moves the reference by more than 4 ulp somewhere - in every family that has a recurrent step
    (max(lens) >= 2; at T = 1 or lens all 1 there is no W_hh term to lose, those families are held by the gate-order
    mutation below) - and so does moving a short sentence's final hidden state to step T-1 in every family that has a short
    sentence. The mutations of the whole recurrence (gate order everywhere, direction-1 position where a sentence has two
    steps) fail BOTH pass criteria of the GPU tests against the unaltered reference; the final-hidden step, which touches
    only the final rows of the short sentences, fails (a) on the whole output and (b) on the final rows. (At R = 1024 the two
    re-runs of the recurrence are made at T <= 4 and at one T = 20 family per Bn: 67 MB of float64 weights per step.)
    The inputs are the draws the GPU tests use (lstm_ref.family_case: the first draw on which four perturbed float32
    evaluations stay within half the (b) bound)."""
    w64, w0 = lr.prepped_whh(R, dtype), lr.prepped_whh(R, dtype, zero_slice=True)
    worst_noise, worst_share, least_sens, draws = 0.0, 0.0, float("inf"), 0
    for (_, _, T, kind, lens) in [f for f in _families(R) if f[1] == Bn]:
        cs = lr.family_case(R, Bn, T, kind, lens, dtype)          # (a draw on which criterion (b) is settled: lstm_ref.settled)
        gx, r64, noise, share = cs["gx"], cs["r64"], cs["noise"], cs["pair"]
        o64 = r64[:Bn * T].reshape(Bn, T, 2 * R)
        mask = lr.active_mask(lens, T, R)
        draws = max(draws, cs["draw"])
        worst_noise, worst_share = max(worst_noise, noise), max(worst_share, share)
        assert noise <= 1.0, (R, Bn, T, lens, noise)
        bound = lr.share_bound(share)
        rerun = R < 1024 or T <= 4 or kind == "mix" or Bn == 1

        def fails_both(o, f, what):
            dv, sh = lr.deviation(lr.stack_rows(o, f), r64, dtype, mask)
            assert dv > lr.MAX_ULP and sh > bound, (what, R, Bn, T, lens, dv, sh, bound)

        if rerun:
            fails_both(*lr.bilstm_ref(gx, w64, lens, dtype, gate_order=(1, 0, 2, 3)), "gate order")
        if max(lens) >= 2:
            sens, _ = lr.deviation(lr.stack_rows(*lr.bilstm_ref(gx, w0, lens, dtype)), r64, dtype, mask)
            least_sens = min(least_sens, sens)
            assert sens > 4.0, ("W_hh slice", R, Bn, T, lens, sens)
            if rerun:
                fails_both(*lr.bilstm_ref(gx, w64, lens, dtype, dir1_pos=lambda s, ln: torch.full_like(ln, s)), "direction-1 position")
        if min(lens) < T:
            # touches the final rows of the short sentences only (3 of 69 rows at Bn = 5, T = 20): criterion (a) is the one
            # that has to see it on the whole output; (b) is asserted on the rows the mutation can reach, the final ones
            mut = lr.stack_rows(o64, lr.final_from_last_step(o64, lens))
            dv, _ = lr.deviation(mut, r64, dtype, mask)
            fin = mask.clone()
            fin[:Bn * T] = False
            _, sh = lr.deviation(mut, r64, dtype, fin)
            assert dv > 4.0 and sh > bound, ("final-hidden step", R, Bn, T, lens, dv, sh, bound)
    print(f"    R={R} Bn={Bn} {dtype}: noise <= {worst_noise:.2f} ulp, unequal share <= {100 * worst_share:.2f} %, "
          f"W_hh-slice sensitivity >= {least_sens:.1f} ulp, re-draws <= {draws}")
