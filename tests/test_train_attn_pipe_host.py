"""The pipelined fused training attention's host side without a GPU: the option value "fused_pipe" (`train.parse_train_attn`,
`extended_config.parse_train_attn`, `check_hip_options`, `trn_utils.train_attn`), the per-thread switch `attn_fused_pipe` and its
launch counter (`vog_train_set_int` / `vog_train_get_int`), and `vog_attn_fused_scratch_bytes`, which does not follow the switch:
the pipelined kernels keep their operand images in LDS."""
import ctypes as C
import importlib
import os
import re
import threading

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
EC = importlib.import_module("vognet-pytorch_amd.extended_config")
TR = importlib.import_module("vognet-pytorch_amd.train")
TU = importlib.import_module("vognet-pytorch_amd.trn_utils")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("flash", "Fused_pipe", "", None)
SHAPES = [(1, 1, 1, 1, 1), (2, 1, 1, 8, 2), (3, 100, 100, 512, 3), (2, 100, 20, 768, 3), (4, 4000, 4000, 512, 3), (40, 2000, 400, 768, 3)]


class Cfg(dict):
    pass


def _get(lib, name):
    v = C.c_int(-7)
    assert lib.vog_train_get_int(name, C.byref(v)) == 0
    return v.value


def test_trainer_parser_accepts_fused_pipe():
    assert TR.parse_train_attn("fused_pipe") == "fused_pipe"
    assert TR.parse_train_attn("fused") == "fused" and TR.parse_train_attn("materialized") == "materialized"
    assert "fused_pipe" in TR.ATTN_MODES and TR.ATTN_MODES[0] == "materialized"
    for bad in BAD:
        with pytest.raises(ValueError):
            TR.parse_train_attn(bad)


def test_cfg_key_accepts_fused_pipe():
    assert EC.parse_train_attn({"train_attn": "fused_pipe"}) == "fused_pipe"
    assert EC.parse_train_attn({}) == "materialized"
    for bad in BAD:
        with pytest.raises(ValueError):
            EC.parse_train_attn({"train_attn": bad})
    EC.check_hip_options(Cfg(hip={"train_attn": "fused_pipe"}))
    for bad in BAD:
        with pytest.raises(ValueError, match="train_attn"):
            EC.check_hip_options(Cfg(hip={"train_attn": bad}))
    assert TU.train_attn(Cfg(hip={"train_attn": "fused_pipe"})) == "fused_pipe"
    assert TU.train_attn(Cfg(hip={"train_attn": "fused"})) == "fused" and TU.train_attn(Cfg()) == "materialized"


def test_default_config_keeps_materialized():
    src = open(os.path.join(ROOT, "vognet-pytorch_amd", "extended_config.py")).read()
    assert re.search(r'"train_attn":\s*"materialized"', src)


def test_switch_sets_reads_back_and_refuses_other_values():
    lib = L.load()
    assert _get(lib, b"attn_fused_pipe") == 0                        # the default
    try:
        assert lib.vog_train_set_int(b"attn_fused_pipe", 1) == 0
        assert _get(lib, b"attn_fused_pipe") == 1
        for bad in (2, -1):
            assert lib.vog_train_set_int(b"attn_fused_pipe", bad) == -1
            assert _get(lib, b"attn_fused_pipe") == 1
        for name in (b"amp", b"bf16_gemm", b"lstm_fused", b"lstm_amp_split", b"gemm_amp_pipe"):
            assert _get(lib, name) == 0, name                        # the neighbours are switches of their own
        assert lib.vog_train_set_int(b"attn_fused_pipe", 0) == 0
        for bad in (2, -1):
            assert lib.vog_train_set_int(b"attn_fused_pipe", bad) == -1
            assert _get(lib, b"attn_fused_pipe") == 0
    finally:
        assert lib.vog_train_set_int(b"attn_fused_pipe", 0) == 0
    assert _get(lib, b"attn_fused_pipe") == 0


def test_counter_reads_zero_and_can_only_be_reset_to_zero():
    lib = L.load()
    assert _get(lib, b"attn_fused_pipe_launches") == 0
    assert lib.vog_train_set_int(b"attn_fused_pipe_launches", 0) == 0
    for bad in (1, -1, 5):
        assert lib.vog_train_set_int(b"attn_fused_pipe_launches", bad) == -1
    assert _get(lib, b"attn_fused_pipe_launches") == 0


def test_defaults_are_zero_in_a_fresh_thread():
    lib = L.load()
    seen = {}
    try:
        assert lib.vog_train_set_int(b"attn_fused_pipe", 1) == 0     # this thread's value does not leak into another's

        def read():
            for name in (b"attn_fused_pipe", b"attn_fused_pipe_launches", b"amp", b"bf16_gemm", b"f32_products", b"lstm_fused",
                         b"lstm_fused_launches", b"lstm_amp_split", b"lstm_amp_split_launches", b"gemm_amp_pipe",
                         b"gemm_amp_pipe_launches"):
                seen[name] = _get(lib, name)

        t = threading.Thread(target=read)
        t.start()
        t.join()
    finally:
        lib.vog_train_set_int(b"attn_fused_pipe", 0)
    assert len(seen) == 11 and all(v == 0 for v in seen.values()), seen


@pytest.mark.parametrize("amp", [0, 1, 2])
@pytest.mark.parametrize("S,N,n,d,H", SHAPES)
def test_scratch_bytes_do_not_follow_the_switch(S, N, n, d, H, amp):
    lib = L.load()
    f = lib.vog_attn_fused_scratch_bytes
    try:
        assert lib.vog_train_set_int(b"amp", amp) == 0
        off = int(f(S, N, n, d, H))
        assert off > 0
        assert lib.vog_train_set_int(b"attn_fused_pipe", 1) == 0
        assert int(f(S, N, n, d, H)) == off
    finally:
        lib.vog_train_set_int(b"amp", 0)
        lib.vog_train_set_int(b"attn_fused_pipe", 0)
