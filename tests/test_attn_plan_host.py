"""Without a GPU: which kernels the two inference attention entries launch (csrc/attention.hip: attn_plan / attn_struct_plan,
exported as vog_attn_plan / vog_attn_struct_plan) against tests/golden/attn_plans.json. The fixture's kernels, template flags,
workgroups, workgroup sizes and return codes were recorded from a kernel trace of the library BEFORE the choice moved into the plan
functions (scratch/attn_launch_rows.py); its dynamic LDS bytes are what that library passed to its launches in a host-only run
(scratch/attn_host_lds.cpp: the trace reports static LDS only), equal to this library's plans when recorded. No operand exists
here: the plans read scalars and test pointers for null."""
import ctypes as C
import importlib
import json
import os

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
FAKE = 0x1000                      # a non-null value for the optional pointers (never dereferenced by a plan)
FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plans.json")))
ROWS = FIX["rows"]


def _pad(n):
    return (n + 31) // 32 * 32


def _args(r):
    S, H = FIX["S"], FIX["H"]
    if r["e"] == "rel":
        a = L.AttnArgs()
        a.S, a.N, a.H, a.dp, a.npad = S, r["N"], H, r["dp"], _pad(r["N"])
        a.guard_precleared = int(r["guard"] == "precleared")
        if r["split"]:
            a.q_lo, a.k_lo = FAKE, FAKE
    else:
        a = L.AttnStructArgs()
        a.S, a.H, a.dp, a.nsrl, a.nppf = S, H, r["dp"], r["nsrl"], r["nppf"]
        a.npad_q, a.npad_kv, a.q_visual = _pad(r["nsrl"] * r["nppf"]), _pad(r["nppf"]), r["q_visual"]
        if r["split"]:
            a.q_lo, a.kv_lo = FAKE, FAKE
    a.dtype = L.VOG_BF16
    if r["guard"] != "none":
        a.guard_flag = FAKE
    if r["out_lo"]:
        a.out16_lo = FAKE
    return a


def _plan(lib, r):
    out, n = (L.AttnLaunch * 3)(), C.c_int32(-1)
    fn = lib.vog_attn_plan if r["e"] == "rel" else lib.vog_attn_struct_plan
    rc = fn(C.byref(_args(r)), out, C.byref(n))
    return rc, [[lib.vog_attn_kernel_name(out[i].kernel).decode(), out[i].flag, out[i].grid, out[i].block, out[i].lds]
                for i in range(n.value)]


def test_the_table_is_whole():
    rel = [r for r in ROWS if r["e"] == "rel"]
    st = [r for r in ROWS if r["e"] == "struct"]
    assert len(rel) == 5 * 14 * 3 * 2 + 2 and len(st) == 5 * 7 * 5 * 2 * 2 * 2
    assert any(r["rc"] != 0 for r in rel) and any(r["rc"] != 0 for r in st)
    assert all(la[4] is not None for r in ROWS for la in r["launches"])


def test_plans_are_the_recorded_launches():
    lib = L.load()
    bad = []
    for r in ROWS:
        rc, launches = _plan(lib, r)
        if rc != r["rc"] or launches != (r["launches"] if rc == 0 else []):
            bad.append((r, rc, launches))
        assert (rc == 0) == (len(r["launches"]) > 0)
    assert not bad, (len(bad), bad[:3])


def test_guard_lds_cap_and_refusals():
    """What the trace does not show: how each launch gets the guard word, the limit raised for it, and why a shape is refused."""
    lib = L.load()
    for r in ROWS:
        out, n = (L.AttnLaunch * 3)(), C.c_int32(-1)
        fn = lib.vog_attn_plan if r["e"] == "rel" else lib.vog_attn_struct_plan
        rc = fn(C.byref(_args(r)), out, C.byref(n))
        if rc != 0:
            assert rc == -1 and n.value == 0
            msg = lib.vog_last_error().decode()
            assert "LDS budget" in msg or "needs q_visual" in msg or "needs a head dim" in msg, msg
            continue
        names = [lib.vog_attn_kernel_name(out[i].kernel).decode() for i in range(n.value)]
        guards = [out[i].guard for i in range(n.value)]
        two_pass = "attn_tile2_kernel" in names or "attn_struct_ef_kernel" in names
        assert two_pass == (n.value > 1)
        if two_pass:           # [clear,] first pass raising the word, then its gated fallback; only with a guard word
            assert r["guard"] != "none" and guards == [1] * (n.value - 1) + [2]
            assert ("attn_guard_clear_kernel" in names) == (r["e"] == "rel" and r["guard"] == "given")
        else:
            assert guards == [0]
        for i in range(n.value):
            assert out[i].lds <= max(out[i].lds_cap, 64 * 1024) and out[i].lds_cap in (0, 64 << 10, 72 << 10, 80 << 10, 150 << 10, 160 << 10)


def test_every_kernel_of_the_enum_is_in_the_fixture():
    lib = L.load()
    names = set()
    k = 0
    while lib.vog_attn_kernel_name(k) is not None:
        names.add(lib.vog_attn_kernel_name(k).decode())
        k += 1
    assert k == 12 and lib.vog_attn_kernel_name(-1) is None
    assert names == {la[0] for r in ROWS for la in r["launches"]}


def test_support_queries_are_the_hi_lo_plans():
    """attn_split_supported / attn_struct_split_supported (what vog_ctx_split_supported asks per attention step) = the hi + lo
    plan of the shape succeeds."""
    lib = L.load()
    seen = set()
    for r in ROWS:
        if not r["split"] or (r["e"] == "struct" and not r["q_visual"]):
            continue
        key = (r["e"], r["dp"], r.get("N"), r.get("nppf"), r.get("nsrl"))
        if key in seen:
            continue
        seen.add(key)
        rc, _ = _plan(lib, r)
        got = lib.vog_attn_split_supported(r["N"], r["dp"]) if r["e"] == "rel" else \
            lib.vog_attn_struct_split_supported(r["nppf"], r["nsrl"], r["dp"])
        assert got == int(rc == 0) == int(r["rc"] == 0), (r, got, rc)
    assert len(seen) == 5 * 14 + 1 + 5 * 7 * 5
    for dp in (0, 16, 48, 96, 512):
        assert lib.vog_attn_split_supported(100, dp) == 0 and lib.vog_attn_struct_split_supported(20, 5, dp) == 0


@pytest.mark.parametrize("dp,N,want", [(256, 13793, 1), (256, 13824, 1), (256, 13825, 0), (128, 26112, 1), (128, 26113, 0)])
def test_split_supported_at_the_lds_limit(dp, N, want):
    """2 ring slots of 3 * dp / 16 KB + 4 bytes per padded key against 150 KB: 13824 keys at head dim 256, 26112 at 128."""
    assert L.load().vog_attn_split_supported(N, dp) == want
