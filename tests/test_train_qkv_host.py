"""The factored Q / K / V projections of mul_tx's layer 0 without a GPU: the ctypes mirror of `vog_attn_vl` against the C header,
`vog_attn_vl_scratch_bytes` (a layout walked without a base), the argument errors and the short-scratch refusal of the two `_vl`
entries (returned before any device call, so they show on a machine without a device), the option `qkv` / `cfg.hip.train_qkv`
on its three surfaces, and the float64 restatement of the factored forward and backward (tests/qkv_ref.py) against autograd
through the dense operator."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest
import torch

from tests import qkv_ref as Q

L = importlib.import_module("vognet-pytorch_amd.lib")
EC = importlib.import_module("vognet-pytorch_amd.extended_config")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAD, PAD = 255, 16            # csrc/train_dev.h Carve: 4-float carves behind a 256-byte boundary
GOOD = (2, 2, 2, 7, 3, 32, 16, 0)          # n_q, nc_v, nfrm, n, nsrl, dobj, dlang, lang_per_vid


def test_ctypes_struct_matches_the_c_header(tmp_path):
    """sizeof and the offset of every member of vog_attn_vl as the C compiler lays them out."""
    names = [n for n, _ in L.AttnVL._fields_]
    prog = tmp_path / "lay.c"
    lines = "\n".join(f'  printf("{n} %zu\\n", offsetof(vog_attn_vl, {n}));' for n in names)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vog_hip.h"\nint main(void) {\n'
                    '  printf("sizeof %zu\\n", sizeof(vog_attn_vl));\n' + lines + "\n  return 0;\n}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.AttnVL)
    for n in names:
        assert int(out[n]) == getattr(L.AttnVL, n).offset, n
    assert int(out["ps"]) == 0 and int(out["scratch_bytes"]) > int(out["scratch"]) > int(out["accumulate"]) > int(out["d_lang"])


def test_scratch_bytes_refuse_non_positive_dimensions():
    f = L.load().vog_attn_vl_scratch_bytes
    assert f(*GOOD) > 0 and f(*GOOD[:7], 1) > 0
    for i in range(7):                                                  # (the eighth is a flag)
        for bad in (0, -1):
            assert f(*(GOOD[:i] + (bad,) + GOOD[i + 1:])) == -1, (i, bad)


def test_scratch_bytes_grow_in_every_dimension_and_follow_the_carve():
    f = L.load().vog_attn_vl_scratch_bytes
    for i in range(7):
        sizes = [int(f(*(GOOD[:i] + (v,) + GOOD[i + 1:]))) for v in (1, 3, 8, 65)]
        for nb in sizes:
            assert nb >= LEAD and (nb - LEAD) % PAD == 0, (i, nb)
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (i, sizes)
    # exactly: Pv and dPv [S*n, d], Pl and dPl [G*nsrl, d], the per-sequence sums [S*nsrl, d], three of each
    n_q, nc_v, nfrm, n, nsrl, dobj, dlang, _ = GOOD
    r16 = lambda b: (b + 15) // 16 * 16
    for lpv in (0, 1):
        S, G, d = n_q * nc_v * nfrm, n_q * (nc_v if lpv else 1), dobj + dlang
        want = LEAD + 3 * (2 * r16(S * n * d * 4) + 2 * r16(G * nsrl * d * 4) + r16(S * nsrl * d * 4))
        assert int(f(*GOOD[:7], lpv)) == want
    assert int(f(*GOOD[:7], 1)) > int(f(*GOOD[:7], 0))                   # one argument row per video instead of per query


def _args(cls, shape=GOOD, H=3):
    """An argument struct and a descriptor that pass every check, on made-up addresses: nothing may dereference them."""
    lib = L.load()
    n_q, nc_v, nfrm, n, nsrl, dobj, dlang, lpv = shape
    S, N, d = n_q * nc_v * nfrm, nsrl * n, dobj + dlang
    a, v = cls(), L.AttnVL()
    a.wq, a.wk, a.wv, a.cat_out, a.scratch = 0x1000, 0x2000, 0x3000, 0x4000, 0x100000
    a.S, a.N, a.n, a.d, a.n_heads = S, N, n, d, H
    a.scratch_bytes = int(lib.vog_attn_fused_scratch_bytes(S, N, n, d, H) if cls is L.AttnFusedArgs else
                          lib.vog_attn_f32_scratch_bytes(S, N, n, d))
    v.ps, v.lang, v.scratch = 0x5000, 0x6000, 0x200000
    v.n_q, v.nc_v, v.nfrm, v.nsrl, v.dobj, v.dlang, v.lang_per_vid = n_q, nc_v, nfrm, nsrl, dobj, dlang, lpv
    v.scratch_bytes = int(lib.vog_attn_vl_scratch_bytes(*shape))
    return a, v


@pytest.mark.parametrize("entry,cls", [("vog_attn_f32_vl", L.AttnF32Args), ("vog_attn_fused_f32_vl", L.AttnFusedArgs)])
def test_argument_errors_and_short_scratch_come_before_any_device_call(entry, cls):
    """-1 / -2 from made-up pointers on a machine that may have no device: a launch or a copy would give a HIP error code
    (below -1000) or fault on the addresses."""
    fn = getattr(L.load(), entry)

    def run(edit):
        a, v = _args(cls)
        edit(a, v)
        return fn(C.byref(a), C.byref(v), None)

    assert run(lambda a, v: setattr(v, "dlang", 0)) == -1                               # no language part
    assert run(lambda a, v: setattr(a, "d_x", 0x7000)) == -1                            # d_x set
    assert run(lambda a, v: setattr(a, "S", a.S + 1)) == -1                             # geometry: S
    assert run(lambda a, v: setattr(v, "nsrl", v.nsrl + 1)) == -1                       # geometry: N
    assert run(lambda a, v: setattr(v, "dobj", v.dobj + 4)) == -1                       # geometry: d
    assert run(lambda a, v: setattr(v, "ps", None)) == -1
    assert run(lambda a, v: setattr(v, "scratch_bytes", v.scratch_bytes - 1)) == -2     # the descriptor's scratch, one byte short
    assert run(lambda a, v: setattr(a, "scratch_bytes", a.scratch_bytes - 1)) == -2     # the operator's own
    assert fn(C.byref(_args(cls)[0]), None, None) == -1                                 # no descriptor: the dense entry's job


def test_counter_is_read_only_and_resets():
    lib = L.load()
    v = C.c_int32(-1)
    assert lib.vog_train_get_int(b"attn_vl_launches", C.byref(v)) == 0 and v.value == 0
    assert lib.vog_train_set_int(b"attn_vl_launches", 0) == 0
    assert lib.vog_train_set_int(b"attn_vl_launches", 1) == -1
    assert lib.vog_train_get_int(b"attn_vl_launches", C.byref(v)) == 0 and v.value == 0


def test_option_is_parsed_on_every_surface():
    TR = importlib.import_module("vognet-pytorch_amd.train")
    TU = importlib.import_module("vognet-pytorch_amd.trn_utils")
    assert TR.parse_train_qkv("dense") == "dense" and TR.parse_train_qkv("factored") == "factored"
    for bad in ("", "Factored", "fused", None, 1):
        with pytest.raises(ValueError, match="qkv"):
            TR.parse_train_qkv(bad)
        with pytest.raises(ValueError, match="qkv"):                    # the constructor checks it before it needs anything else
            TR.FP32Trainer(None, None, {}, None, qkv=bad)
        with pytest.raises(ValueError, match="train_qkv"):
            EC.parse_train_qkv({"train_qkv": bad})
    assert EC.parse_train_qkv({}) == "dense" and EC.parse_train_qkv({"train_qkv": "factored"}) == "factored"

    class Cfg(dict):
        pass

    EC.check_hip_options(Cfg(hip={"train_qkv": "factored"}))
    EC.check_hip_options(Cfg(hip={}))
    with pytest.raises(ValueError, match="train_qkv"):
        EC.check_hip_options(Cfg(hip={"train_qkv": "Factored"}))
    assert TU.train_qkv(Cfg(hip={"train_qkv": "factored"})) == "factored" and TU.train_qkv(Cfg()) == "dense"
    src = open(os.path.join(ROOT, "vognet-pytorch_amd", "extended_config.py")).read()
    assert re.search(r'"train_qkv":\s*"dense"', src)
    # the autograd path reads the key where it reads train_attn
    src = open(os.path.join(ROOT, "vognet-pytorch_amd", "autograd.py")).read()
    assert re.search(r"tr\.qkv = parse_train_qkv\(hip\)", src)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", Q.SHAPES)
def test_float64_restatement_equals_autograd_through_the_dense_operator(shape, masked):
    """The algebra the kernels implement, in float64 where only the order of the sums differs: 1e-9 of each tensor's largest
    entry (2^-53 times the few hundred terms of the longest sum is below 1e-13)."""
    c = Q.case(shape, masked)
    ref, got = Q.dense(c, torch.float64), Q.factored(c, torch.float64)
    for k, r in ref.items():
        if r is None:
            assert got[k] is None
            continue
        err = float((got[k] - r).abs().max()) / max(float(r.abs().max()), 1e-300)
        assert err <= 1e-9, (k, err)
    if masked:
        m = c["msk"].bool()
        assert not m[:c["G"] // shape[0] * c["nsrl"]].any() and float(ref["d_lang"][~m].abs().max()) == 0.0


def test_dense_reference_is_the_operator_tests_reference():
    """`qkv_ref.dense`'s own attention against `_attn_ref` of tests/test_gpu_bwd_ops.py, the reference the issue names."""
    from tests.test_gpu_bwd_ops import _attn_ref
    c = Q.case(Q.SHAPES[1], True)
    a, b = Q.dense(c, torch.float64), Q.dense(c, torch.float64, attn=_attn_ref)
    for k in a:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * float(b[k].abs().max()), k
