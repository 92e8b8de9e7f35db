"""The fused fp32 BiLSTM recurrence's host side without a GPU: the per-thread switch `lstm_fused` and its launch counter
(`vog_train_set_int` / `vog_train_get_int`), `vog_lang_f32_scratch_bytes` under the switch (a layout walked without a base, no
kernel runs), and the cfg key `hip.train_lstm`."""
import ctypes as C
import importlib
import os
import re

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
EC = importlib.import_module("vognet-pytorch_amd.extended_config")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 7, 3, 8, 4, 2, 40, 5), (4, 12, 3, 32, 1024, 2, 48, 40), (24, 7, 3, 8, 16, 4, 6, 5), (1, 1, 1, 1, 1, 1, 1, 1)]


def _get(lib, name):
    v = C.c_int(-7)
    assert lib.vog_train_get_int(name, C.byref(v)) == 0
    return v.value


def test_cfg_key_is_parsed_and_checked():
    assert EC.parse_train_lstm({}) == "stepwise"
    assert EC.parse_train_lstm({"train_lstm": "stepwise"}) == "stepwise"
    assert EC.parse_train_lstm({"train_lstm": "fused"}) == "fused"
    for bad in ("", "persistent", None, 1):
        with pytest.raises(ValueError):
            EC.parse_train_lstm({"train_lstm": bad})

    class Cfg(dict):
        pass

    EC.check_hip_options(Cfg(hip={"train_lstm": "fused"}))
    EC.check_hip_options(Cfg(hip={}))
    with pytest.raises(ValueError, match="train_lstm"):
        EC.check_hip_options(Cfg(hip={"train_lstm": "Fused"}))
    TR = importlib.import_module("vognet-pytorch_amd.train")
    assert TR.parse_train_lstm("fused") == "fused" and TR.parse_train_lstm("stepwise") == "stepwise"
    with pytest.raises(ValueError):
        TR.parse_train_lstm("persistent")
    TU = importlib.import_module("vognet-pytorch_amd.trn_utils")
    assert TU.train_lstm(Cfg(hip={"train_lstm": "fused"})) == "fused" and TU.train_lstm(Cfg()) == "stepwise"


def test_default_config_carries_the_key():
    src = open(os.path.join(ROOT, "vognet-pytorch_amd", "extended_config.py")).read()
    assert re.search(r'"train_lstm":\s*"stepwise"', src)


def test_switch_sets_reads_back_and_refuses_other_values():
    lib = L.load()
    assert _get(lib, b"lstm_fused") == 0                             # the default
    try:
        assert lib.vog_train_set_int(b"lstm_fused", 1) == 0
        assert _get(lib, b"lstm_fused") == 1
        for bad in (2, -1):
            assert lib.vog_train_set_int(b"lstm_fused", bad) == -1
            assert _get(lib, b"lstm_fused") == 1
        assert _get(lib, b"amp") == 0 and _get(lib, b"bf16_gemm") == 0      # the neighbours are switches of their own
    finally:
        assert lib.vog_train_set_int(b"lstm_fused", 0) == 0
    assert _get(lib, b"lstm_fused") == 0


def test_counter_can_only_be_reset_to_zero():
    lib = L.load()
    assert lib.vog_train_set_int(b"lstm_fused_launches", 0) == 0
    assert _get(lib, b"lstm_fused_launches") == 0
    for bad in (1, -1, 5):
        assert lib.vog_train_set_int(b"lstm_fused_launches", bad) == -1
    assert _get(lib, b"lstm_fused_launches") == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_scratch_bytes_follow_the_switch(shape):
    lib = L.load()
    f = lib.vog_lang_f32_scratch_bytes
    before = int(f(*shape))
    assert before > 0
    Bn, T, nsrl, E, R, layers, D, Lo = shape
    try:
        assert lib.vog_train_set_int(b"lstm_fused", 1) == 0
        on = int(f(*shape))
        # the second direction's dG by step and by position, its dc and its W_hh^T, each padded to 64 floats (csrc/train_dev.h)
        pad = lambda n: (n * 4 + 255) // 256 * 256
        assert on == before + 2 * pad(Bn * T * 4 * R) + pad(Bn * R) + pad(4 * R * R)
        for i in range(len(shape)):
            for bad in (0, -1):
                assert f(*(shape[:i] + (bad,) + shape[i + 1:])) == -1, (i, bad)
        assert f(*(shape[:5] + (5,) + shape[6:])) == -1                 # at most 4 layers
        # amp has fused kernels and a layout of its own: the switch changes nothing there
        assert lib.vog_train_set_int(b"amp", 1) == 0
        amp_on = int(f(*shape))
        assert lib.vog_train_set_int(b"lstm_fused", 0) == 0
        assert int(f(*shape)) == amp_on
    finally:
        lib.vog_train_set_int(b"amp", 0)
        lib.vog_train_set_int(b"lstm_fused", 0)
    assert int(f(*shape)) == before


# vog_lang_f32_scratch_bytes at SHAPES under (amp, lstm_fused) = (0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), recorded from the
# build before the recurrence kernels and the layout's carves of dGs1 / dGp1 / dc1 were merged: no carve moved or changed size
SCRATCH_BYTES = [[54527, 58111, 59903, 59903, 59903, 59903],
                 [29212927, 47579391, 97913087, 97913087, 97913087, 97913087],
                 [1168639, 1260287, 1293055, 1293055, 1293055, 1293055],
                 [9471, 10495, 11263, 11263, 11263, 11263]]


@pytest.mark.parametrize("shape,want", list(zip(SHAPES, SCRATCH_BYTES)))
def test_scratch_bytes_are_the_recorded_ones(shape, want):
    lib = L.load()
    try:
        got = []
        for amp in (0, 1, 2):
            for fused in (0, 1):
                assert lib.vog_train_set_int(b"amp", amp) == 0 and lib.vog_train_set_int(b"lstm_fused", fused) == 0
                got.append(int(lib.vog_lang_f32_scratch_bytes(*shape)))
    finally:
        lib.vog_train_set_int(b"amp", 0)
        lib.vog_train_set_int(b"lstm_fused", 0)
    assert got == want
