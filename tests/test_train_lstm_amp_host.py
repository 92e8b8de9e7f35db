"""The K-split mixed-precision BiLSTM recurrence's host side without a GPU: the per-thread switch `lstm_amp_split` and its launch
counter (`vog_train_set_int` / `vog_train_get_int`), `vog_lang_f32_scratch_bytes` (which does not follow the switch: the split
kernels keep the tile kernels' buffers), and the cfg key `hip.train_lstm_amp`."""
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


def test_switch_sets_reads_back_and_refuses_other_values():
    lib = L.load()
    assert _get(lib, b"lstm_amp_split") == 0                         # the default
    try:
        assert lib.vog_train_set_int(b"lstm_amp_split", 1) == 0
        assert _get(lib, b"lstm_amp_split") == 1
        for bad in (2, -1):
            assert lib.vog_train_set_int(b"lstm_amp_split", bad) == -1
            assert _get(lib, b"lstm_amp_split") == 1
        # the neighbours are switches of their own
        assert _get(lib, b"amp") == 0 and _get(lib, b"bf16_gemm") == 0 and _get(lib, b"lstm_fused") == 0
    finally:
        assert lib.vog_train_set_int(b"lstm_amp_split", 0) == 0
    assert _get(lib, b"lstm_amp_split") == 0


def test_counter_can_only_be_reset_to_zero():
    lib = L.load()
    assert lib.vog_train_set_int(b"lstm_amp_split_launches", 0) == 0
    assert _get(lib, b"lstm_amp_split_launches") == 0
    for bad in (1, -1, 5):
        assert lib.vog_train_set_int(b"lstm_amp_split_launches", bad) == -1
    assert _get(lib, b"lstm_amp_split_launches") == 0


@pytest.mark.parametrize("amp", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_scratch_bytes_do_not_follow_the_switch(shape, amp):
    lib = L.load()
    f = lib.vog_lang_f32_scratch_bytes
    try:
        assert lib.vog_train_set_int(b"amp", amp) == 0
        off = int(f(*shape))
        assert off > 0
        assert lib.vog_train_set_int(b"lstm_amp_split", 1) == 0
        assert int(f(*shape)) == off
    finally:
        lib.vog_train_set_int(b"amp", 0)
        lib.vog_train_set_int(b"lstm_amp_split", 0)


def test_cfg_key_is_parsed_and_checked():
    assert EC.parse_train_lstm_amp({}) == "tile"
    assert EC.parse_train_lstm_amp({"train_lstm_amp": "tile"}) == "tile"
    assert EC.parse_train_lstm_amp({"train_lstm_amp": "split"}) == "split"
    for bad in ("", "Split", None, 1):
        with pytest.raises(ValueError):
            EC.parse_train_lstm_amp({"train_lstm_amp": bad})

    class Cfg(dict):
        pass

    EC.check_hip_options(Cfg(hip={"train_lstm_amp": "split"}))
    EC.check_hip_options(Cfg(hip={}))
    with pytest.raises(ValueError, match="train_lstm_amp"):
        EC.check_hip_options(Cfg(hip={"train_lstm_amp": "Split"}))
    TU = importlib.import_module("vognet-pytorch_amd.trn_utils")
    assert TU.train_lstm_amp(Cfg(hip={"train_lstm_amp": "split"})) == "split" and TU.train_lstm_amp(Cfg()) == "tile"


def test_default_config_carries_the_key():
    src = open(os.path.join(ROOT, "vognet-pytorch_amd", "extended_config.py")).read()
    assert re.search(r'"train_lstm_amp":\s*"tile"', src)


def test_trainer_parser_refuses_other_strings():
    TR = importlib.import_module("vognet-pytorch_amd.train")
    assert TR.parse_train_lstm_amp("split") == "split" and TR.parse_train_lstm_amp("tile") == "tile"
    for bad in ("", "Split", "fused", None, 1):
        with pytest.raises(ValueError):
            TR.parse_train_lstm_amp(bad)
