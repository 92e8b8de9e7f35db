"""Host half of the wide BiLSTM layer kernel's tests (no GPU): the two new entries are exported and declared, the
`vog_bilstm_layer_wide_supported` truth table, the `cfg.hip.lstm_wide` switch, and the conditions the float64 restatement of
tests/lstm_ref.py alone has to meet at the shapes tests/test_gpu_lstm_wide.py holds the kernel to criteria (a) and (b) on."""
import importlib
import os
import re

import pytest

from tests import lstm_ref as lr

L = importlib.import_module("vognet-pytorch_amd.lib")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (R, Bn, T) of the criteria test of tests/test_gpu_lstm_wide.py; lens = lstm_ref.make_lens("mix", Bn, T)
WIDE_CRIT = [(R, 32, 20) for R in (128, 1024)]


def test_wide_entries_are_exported_and_declared():
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vog_hip.h")).read()
    for name in ("vog_bilstm_layer_wide_supported", "vog_bilstm_layer_wide"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/vog_hip.h"
        assert getattr(lib, name) is not None, name
    assert "lstm_wide" in src                                   # the context option is documented with the others


def test_wide_supported_truth_table():
    """1 exactly for 17 <= Bn <= 32 under the R rule of the narrow kernel (R / 32 in {1, 2, 4, 32}); the narrow predicate is
    unchanged: it still ends at 16 sentences"""
    lib = L.load()
    for R in (0, 16, 32, 64, 96, 128, 256, 1024, 2080):
        r_ok = R in (32, 64, 128, 1024)
        for Bn in range(35):
            assert bool(lib.vog_bilstm_layer_wide_supported(Bn, R)) == (17 <= Bn <= 32 and r_ok), (Bn, R)
            assert bool(lib.vog_bilstm_layer_supported(Bn, R)) == (1 <= Bn <= 16 and r_ok), (Bn, R)
    assert not lib.vog_bilstm_layer_wide_supported(-1, 32)


def test_hx_bytes_at_32_sentences():
    """[T][2][Bn][R] 16-bit values: what the wide kernel's slots take"""
    lib = L.load()
    assert lib.vog_bilstm_hx_bytes(32, 24, 1024) == 24 * 2 * 32 * 1024 * 2
    assert lib.vog_bilstm_hx_bytes(17, 1, 32) == 2 * 17 * 32 * 2


def test_cfg_switch_parses_and_defaults_to_off():
    cfg = ec.get_default_cfg()
    assert cfg.hip.lstm_wide is False
    ec.update_from_dict(cfg, {"hip.lstm_wide": True})
    assert cfg.hip.lstm_wide is True
    ec.check_hip_options(cfg)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("R,Bn,T", WIDE_CRIT)
def test_restatement_pair_inside_the_bounds(R, Bn, T, dtype):
    """The float64 restatement against its float32-permuted evaluation, on the inputs the GPU test uses (the first draw that
    lstm_ref.settled accepts): at most 1 ulp apart anywhere - half of criterion (a)'s 2 ulp - and, trivially by its
    construction, inside criterion (b)'s bound of 4 x its own share (floor 1 %). Both tiles hold a sentence of length T; the
    ragged lengths of make_lens reach 1."""
    lens = lr.make_lens("mix", Bn, T)
    assert T in lens[:16] and T in lens[16:] and 1 in lens
    cs = lr.family_case(R, Bn, T, "mix", lens, dtype)
    bound = lr.share_bound(cs["pair"])
    print(f"    R={R} Bn={Bn} T={T} {dtype}: draw {cs['draw']}, pair {cs['noise']:.2f} ulp, unequal {100 * cs['pair']:.3f} % (bound {100 * bound:.2f} %)")
    assert cs["noise"] <= 1.0 < lr.MAX_ULP
    assert cs["pair"] <= bound / lr.SHARE_FACTOR
    assert cs["r64"].shape == (Bn * T + Bn, 2 * R)
