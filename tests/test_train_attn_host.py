"""The fused training attention's host side without a GPU: `vog_attn_fused_scratch_bytes` (a layout walked without a base, no
kernel runs), the cfg key `hip.train_attn`, and the ctypes struct against the C header."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
EC = importlib.import_module("vognet-pytorch_amd.extended_config")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAD, PAD = 255, 16            # csrc/train_dev.h Carve: 4-float carves behind a 256-byte boundary, as vog_attn_f32


def test_scratch_bytes_refuse_non_positive_dimensions():
    f = L.load().vog_attn_fused_scratch_bytes
    good = (2, 6, 3, 8, 2)
    assert f(*good) > 0
    for i in range(len(good)):
        for bad in (0, -1):
            assert f(*(good[:i] + (bad,) + good[i + 1:])) == -1, (i, bad)


@pytest.mark.parametrize("amp", [0, 1, 2])
def test_sizes_are_monotone_follow_the_padding_rule_and_ignore_amp(amp):
    lib = L.load()
    f = lib.vog_attn_fused_scratch_bytes
    base = (3, 3, 3, 8, 2)
    off = [[int(f(*(base[:i] + (v,) + base[i + 1:]))) for v in (1, 3, 8, 65)] for i in range(len(base))]
    assert lib.vog_train_set_int(b"amp", amp) == 0
    try:
        for i in range(len(base)):
            sizes = [int(f(*(base[:i] + (v,) + base[i + 1:]))) for v in (1, 3, 8, 65)]
            for nb in sizes:
                assert nb >= LEAD and (nb - LEAD) % PAD == 0, (i, nb)
            assert sizes == sorted(sizes) and sizes == off[i], (i, sizes)
    finally:
        lib.vog_train_set_int(b"amp", 0)


@pytest.mark.parametrize("d,H", [(512, 3), (768, 3)])
@pytest.mark.parametrize("N", [200, 2000, 4000])
def test_scratch_is_linear_in_the_sequence_length(N, d, H):
    lib = L.load()
    f, m = lib.vog_attn_fused_scratch_bytes, lib.vog_attn_f32_scratch_bytes
    for S, n_of in ((4, lambda k: k), (40, lambda k: k // 5)):                  # obj_tx (n = N) and mul_tx (5 argument blocks)
        one, two = int(f(S, N, n_of(N), d, H)), int(f(S, 2 * N, n_of(2 * N), d, H))
        assert 0 < one < two <= 2 * one, (S, N, d, one, two)
        assert int(m(S, 2 * N, n_of(2 * N), d)) > 2 * int(m(S, N, n_of(N), d))      # the materialised operator's is quadratic
    # exactly: 7 [S*N, d] matrices, the boxes, delta and lse [S, H, N], 8 floats per (head, sequence, 64-row tile)
    S, n = 4, N
    r16 = lambda b: (b + 15) // 16 * 16
    want = LEAD + 7 * r16(S * N * d * 4) + r16(S * n * 32) + 2 * r16(S * H * N * 4) + r16(H * S * ((N + 63) // 64) * 32)
    assert int(f(S, N, n, d, H)) == want


def test_cfg_key_is_parsed_and_checked():
    assert EC.parse_train_attn({}) == "materialized"
    assert EC.parse_train_attn({"train_attn": "fused"}) == "fused"
    for bad in ("", "flash", None, 1):
        with pytest.raises(ValueError):
            EC.parse_train_attn({"train_attn": bad})

    class Cfg(dict):
        pass

    EC.check_hip_options(Cfg(hip={"train_attn": "fused"}))
    EC.check_hip_options(Cfg(hip={}))
    with pytest.raises(ValueError, match="train_attn"):
        EC.check_hip_options(Cfg(hip={"train_attn": "Fused"}))
    TR = importlib.import_module("vognet-pytorch_amd.train")
    assert TR.parse_train_attn("fused") == "fused"
    with pytest.raises(ValueError):
        TR.parse_train_attn("flash")
    TU = importlib.import_module("vognet-pytorch_amd.trn_utils")
    assert TU.train_attn(Cfg(hip={"train_attn": "fused"})) == "fused" and TU.train_attn(Cfg()) == "materialized"


def test_default_config_carries_the_key():
    src = open(os.path.join(ROOT, "vognet-pytorch_amd", "extended_config.py")).read()
    assert re.search(r'"train_attn":\s*"materialized"', src)


def test_ctypes_struct_matches_the_c_header(tmp_path):
    """sizeof and the offset of every member of vog_attn_fused_args as the C compiler lays them out."""
    names = [n for n, _ in L.AttnFusedArgs._fields_]
    assert names[:len(L.AttnF32Args._fields_)] == [n for n, _ in L.AttnF32Args._fields_] and names[-3:] == ["lse", "cat", "kept_forward"]
    prog = tmp_path / "lay.c"
    lines = "\n".join(f'  printf("{n} %zu\\n", offsetof(vog_attn_fused_args, {n}));' for n in names)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vog_hip.h"\nint main(void) {\n'
                    '  printf("sizeof %zu\\n", sizeof(vog_attn_fused_args));\n' + lines + "\n  return 0;\n}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.AttnFusedArgs)
    for n in names:
        assert int(out[n]) == getattr(L.AttnFusedArgs, n).offset, n
    assert int(out["x"]) == 0 and int(out["kept_forward"]) > int(out["cat"]) > int(out["lse"]) > int(out["drop_site"])
