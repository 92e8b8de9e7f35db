"""Which kernels the two inference attention entries launch, shape by shape (attn_plan: csrc/attention.hip attn_plan /
attn_struct_plan; the fixture tests/golden/attn_plans.json and profiles/attn_plan_launches.json come from here).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python scratch/attn_launch_rows.py RUN.json
    python scratch/attn_launch_rows.py --fold DIR/.../r_kernel_trace.csv RUN.json LISTING.json
    python scratch/attn_launch_rows.py --rows > ROWS.txt; scratch/attn_host_lds PARENT_LIB.so < ROWS.txt > PARENT_LDS.txt   (attn_host_lds.cpp)
    python scratch/attn_launch_rows.py --fixture PARENT_LISTING.json NEW_LISTING.json tests/golden/attn_plans.json PARENT_LDS.txt

The run drives every row of TABLE through vog_rel_attention_fwd / vog_rel_attention_struct_fwd on zero-filled operands (numbers
are the operator tests' business), S = 2 and H = 1, in one process; the library is VOG_HIP_LIB or the tree's own, opened directly
(a parent build lacks the plan exports that lib.load() types). A torch fill launch in front of every row separates the rows in the
trace. --fold turns a trace into one entry per row: the return code, the launches as (kernel function name without namespace,
template flag, workgroups, workgroup size) and the trace's LDS figure per launch (measured: the kernel's static LDS, 0 for all of
these, so it says nothing about the dynamic bytes). --fixture takes the folded listing of the PARENT's library and of the new one,
requires them equal entry by entry, and writes the rows with the parent's launches plus the dynamic LDS bytes that the parent's
library passed to its launches in a host-only run (attn_host_lds.cpp), required equal to the new library's plan."""
import csv
import ctypes as C
import importlib
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, H = 2, 1
DPS = (32, 64, 128, 192, 256)
GUARDS = ("none", "given", "precleared")


def table():
    rows = []
    for dp, N, guard, split in itertools.product(DPS, (1, 32, 33, 128, 129, 224, 256, 257, 300, 511, 512, 1023, 1024, 4000), GUARDS, (0, 1)):
        rows.append({"e": "rel", "dp": dp, "N": N, "guard": guard, "split": split, "out_lo": split})
    rows.append({"e": "rel", "dp": 64, "N": 200, "guard": "none", "split": 0, "out_lo": 1})      # out16_lo without q_lo
    rows.append({"e": "rel", "dp": 256, "N": 16000, "guard": "none", "split": 1, "out_lo": 1})   # 160 KB against the 150 KB limit
    for dp, nppf, nsrl, qv, guard, split in itertools.product(DPS, (7, 32, 33, 100, 400, 512, 513), (1, 5, 8, 16, 17), (0, 1),
                                                              GUARDS[:2], (0, 1)):
        rows.append({"e": "struct", "dp": dp, "nppf": nppf, "nsrl": nsrl, "q_visual": qv, "guard": guard, "split": split,
                     "out_lo": split})
    return rows


def fill_args(L, r, ptr_in, ptr_out, ptr_out_lo, ptr_guard):
    """The argument block of a row; the pointers are device addresses for the run, any non-null value for a plan call."""
    pad = lambda n: (n + 31) // 32 * 32
    if r["e"] == "rel":
        a = L.AttnArgs()
        a.q, a.k, a.vt, a.out16 = ptr_in, ptr_in, ptr_in, ptr_out
        a.S, a.N, a.H, a.dp, a.npad, a.use_rel, a.n_box, a.seq_per_vid, a.NP = S, r["N"], H, r["dp"], pad(r["N"]), 0, r["N"], 1, r["N"]
        a.guard_precleared = int(r["guard"] == "precleared")
        if r["split"]:
            a.q_lo, a.k_lo = ptr_in, ptr_in
    else:
        a = L.AttnStructArgs()
        a.q, a.kv, a.vv, a.pl, a.out16 = ptr_in, ptr_in, ptr_in, ptr_in, ptr_out
        a.S, a.H, a.dp, a.nsrl, a.nppf = S, H, r["dp"], r["nsrl"], r["nppf"]
        a.npad_q, a.npad_kv, a.nfrm, a.lang_per_vid, a.nc_v = pad(r["nsrl"] * r["nppf"]), pad(r["nppf"]), S, 0, 1
        a.use_rel, a.seq_per_vid, a.NP, a.q_visual = 0, S, S * r["nppf"], r["q_visual"]
        if r["split"]:
            a.q_lo, a.kv_lo = ptr_in, ptr_in
    a.inv_scale, a.dtype = 0.125, L.VOG_BF16
    if r["guard"] != "none":
        a.guard_flag = ptr_guard
    if r["out_lo"]:
        a.out16_lo = ptr_out_lo
    return a


def run(out_path):
    import torch
    L = importlib.import_module("vognet-pytorch_amd.lib")
    lib = C.CDLL(L.LIB_PATH)
    for fn in (lib.vog_rel_attention_fwd, lib.vog_rel_attention_struct_fwd):
        fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    nbytes = 32 << 20            # the largest row reads 16.4 MB per operand and writes 8.9 MB
    zin = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out, out_lo = torch.empty_like(zin), torch.empty_like(zin)
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rcs = []
    for r in table():
        guard.zero_()            # the row separator of the trace (and what guard_precleared promises)
        a = fill_args(L, r, zin.data_ptr(), out.data_ptr(), out_lo.data_ptr(), guard.data_ptr())
        fn = lib.vog_rel_attention_fwd if r["e"] == "rel" else lib.vog_rel_attention_struct_fwd
        rcs.append(int(fn(C.byref(a), L.stream_ptr())))
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"lib": L.LIB_PATH, "rc": rcs}, f)
    print(f"{len(rcs)} rows, {sum(1 for x in rcs if x)} refused")


def fold(trace, run_path, out_path):
    rcs = json.load(open(run_path))["rc"]
    recs = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    lds_col = [c for c in recs[0] if c.upper().startswith("LDS")][0]
    groups, cur = [], None
    for r in recs:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        if "vog::" not in name.split("<")[0]:
            cur = []
            groups.append(cur)
            continue
        assert cur is not None, "a library kernel in front of the first separator"
        m = re.match(r"vog::(\w+)(?:<(.*)>)?\(", name) or re.match(r"vog::(\w+)(?:<(.*)>)?$", name)
        targs = [t.strip() for t in (m.group(2) or "").split(",")]
        flag = {"true": 1, "false": 0}.get(targs[2], targs[2]) if len(targs) == 3 else 0
        wg, grid = int(r["Workgroup_Size_X"]), int(r["Grid_Size_X"])
        assert grid % wg == 0
        cur.append(([m.group(1), int(flag), grid // wg, wg], int(r[lds_col])))
    groups = groups[len(groups) - len(rcs):]          # the separators in front of those are the allocations' fills
    assert len(groups) == len(rcs), (len(groups), len(rcs))
    listing = [{"rc": rc, "launches": [g[0] for g in grp], "lds_trace": [g[1] for g in grp]} for rc, grp in zip(rcs, groups)]
    json.dump(listing, open(out_path, "w"))
    print(f"{len(listing)} rows, {sum(len(e['launches']) for e in listing)} launches")


def plan_of(L, lib, r):
    """(rc, launches) of the library's plan for a row; optional pointers are fake non-null values."""
    a = fill_args(L, r, 64, 64, 64, 64)
    out, n = (L.AttnLaunch * 3)(), C.c_int32(0)
    fn = lib.vog_attn_plan if r["e"] == "rel" else lib.vog_attn_struct_plan
    rc = fn(C.byref(a), out, C.byref(n))
    return rc, [out[i] for i in range(n.value)]


def print_rows():
    """The table as lines for scratch/attn_host_lds.cpp."""
    for r in table():
        g = [int(r["guard"] != "none")] + ([int(r["guard"] == "precleared")] if r["e"] == "rel" else [])
        shape = [r["dp"], r["N"]] if r["e"] == "rel" else [r["dp"], r["nppf"], r["nsrl"], r["q_visual"]]
        print(r["e"], *shape, *g, r["split"], r["out_lo"])


def fixture(parent_path, new_path, out_path, host_lds_path):
    """host_lds_path: what scratch/attn_host_lds.cpp printed for the PARENT's library (the trace's LDS figure turned out to be the
    static LDS alone, 0 for every kernel here, so the dynamic bytes of the parent's launches are taken on the host)."""
    parent, new = json.load(open(parent_path)), json.load(open(new_path))
    rows = table()
    host = [[int(x) for x in ln.split()] for ln in open(host_lds_path) if ln.strip()]
    assert len(parent) == len(new) == len(rows) == len(host)
    differ = [i for i, (p, q) in enumerate(zip(parent, new)) if p != q]
    assert not differ, f"{len(differ)} rows differ between the two libraries, first: {rows[differ[0]]} {parent[differ[0]]} {new[differ[0]]}"
    L = importlib.import_module("vognet-pytorch_amd.lib")
    lib = L.load()
    for r, p, h in zip(rows, parent, host):
        rc, launches = plan_of(L, lib, r)
        r["rc"] = p["rc"]
        hl = [h[2 + 3 * i: 5 + 3 * i] for i in range(h[1])]                       # (workgroups, workgroup size, dynamic LDS bytes)
        assert h[0] == p["rc"] and [x[:2] for x in hl] == [la[2:] for la in p["launches"]], (r, p, h)
        # kernel, flag, workgroups, workgroup size: the PARENT's trace; dynamic LDS bytes: the PARENT's launches on the host,
        # accepted where the new library's plan says the same
        assert [x[2] for x in hl] == [int(pl.lds) for pl in launches], (r, hl)
        r["launches"] = [la + [x[2]] for la, x in zip(p["launches"], hl)]
    with open(out_path, "w") as f:
        f.write('{"S": %d, "H": %d, "rows": [\n' % (S, H) + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]}\n")
    print(f"{len(rows)} rows -> {out_path}")


if __name__ == "__main__":
    if sys.argv[1] == "--fold":
        fold(*sys.argv[2:5])
    elif sys.argv[1] == "--fixture":
        fixture(*sys.argv[2:6])
    elif sys.argv[1] == "--rows":
        print_rows()
    else:
        run(sys.argv[1])
