"""Kernel-by-kernel comparison of two device assembly listings of the training sources (train_dedupe: one body per duplicated
kernel). Each side is one or more files from

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -I include <file> -o <file>.s

    python scratch/kernel_diff.py parent.s -- train_gemm.s train_tx.s train_lang.s > profiles/train_dedupe_kernels.md

Per kernel: registers, spills, LDS and private segment from the metadata; whether the instruction stream is the same after
labels and symbols are normalised; if not, the opcodes whose counts differ, leaving out moves, waits, nops and integer address
arithmetic (whatever opcodes occur are compared; the script knows none by name beyond those classes). A renamed kernel is matched
to its parent instance through RENAMED. The last columns are the compiler's own per-kernel summary (architectural registers,
scratch bytes, waves per SIMD) and the counts of the opcode classes that carry the work: MFMA, LDS, global memory, exp / log,
barrier."""
import collections
import re
import subprocess
import sys

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")
# new demangled name -> the parent's
RENAMED = [(r"^skinny_kernel<(\d+), (\d+), float>$", r"skinny_f32_kernel<\1, \2>"),
           (r"^skinny_kernel<(\d+), (\d+), (BF16|F16)>$", r"skinny16_kernel<\1, \2, \3>"),
           # opt_onebody: the walk-based optimiser kernels lost their _ex, the four table structs became OptTab<K, CAP>
           (r"^opt_apply_kernel<OptTab<4, 20>, (\w+), (\d)>$", r"opt_apply_ex_kernel<OptTable, \1, \2>"),
           (r"^opt_apply_kernel<OptTab<5, 16>, (\w+), (\d)>$", r"opt_apply_ex_kernel<OptTableV, \1, \2>"),
           (r"^opt_stats_kernel<OptTab<4, 20> >$", r"opt_stats_ex_kernel<OptTable>"),
           (r"^opt_stats_kernel<OptTab<5, 16> >$", r"opt_stats_ex_kernel<OptTableV>")]
INFO = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")
CLASSES = (("mfma", r"^v_mfma"), ("lds", r"^ds_"), ("global", r"^(global|flat|buffer)_"), ("exp/log", r"^v_(exp|log)"), ("barrier", r"^s_barrier"))
# not counted: moves, waits, nops, and the integer adds / shifts / multiply-adds that form addresses and indices
UNCOUNTED = re.compile(r"^(v_mov|s_mov|s_waitcnt|s_nop|[vs]_add_(co_)?[iu]|[vs]_addc_|[vs]_sub_(co_)?[iu]|v_subrev_(co_)?[iu]|[vs]_lshl|"
                       r"[vs]_lshr|[vs]_ashr|v_mad_[iu]|v_mul_lo_|v_mul_hi_[iu]|s_mul_i32|s_mul_hi_|v_add3_u|v_add_lshl)")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*\)$", "", d.replace("(anonymous namespace)::", "")).replace("vog::", "").replace("void ", "").strip()
            for n, d in zip(names, out)}


def load(paths):
    kernels = {}
    for path in paths:
        text = open(path).read()
        meta = {}
        for blk in text.split("  - .agpr_count:")[1:]:
            blk = ".agpr_count:" + blk
            get = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
            meta[get("name")] = {k: int(get(k)) for k in META}
        dem = demangle(sorted(meta))
        lines = text.split("\n")
        heads = {ln.split(":")[0]: i for i, ln in enumerate(lines) if ln.startswith("_Z") and ":" in ln}
        for name in meta:
            start = heads[name] + 1
            body = []
            for ln in lines[start:]:
                if ln.startswith(".Lfunc_end"):
                    break
                ln = ln.split(";")[0].strip()
                if ln and not ln.startswith("."):
                    body.append(ln)
                elif ln.startswith(".LBB"):
                    body.append(ln)
            labels = {}
            norm = []
            for ln in body:
                ln = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), ln)
                ln = re.sub(r"_Z\w+", "SYM", ln)
                norm.append(ln)
            for k in INFO:                                      # the "; Kernel info" comments behind the kernel's code
                meta[name][k] = next(int(m.group(1)) for ln in lines[start:] for m in [re.match(r"; %s: (\d+)" % k, ln)] if m)
            kernels[dem[name]] = (meta[name], norm)
    return kernels


def opcounts(body):
    c = collections.Counter()
    for ln in body:
        if ln.endswith(":"):
            continue
        op = ln.split()[0]
        if not UNCOUNTED.match(op):
            c[op] += 1
    return c


def classes(body):
    ops = [ln.split()[0] for ln in body if not ln.endswith(":")]
    return [sum(1 for op in ops if re.match(pat, op)) for _, pat in CLASSES]


def main():
    args = sys.argv[1:]
    cut = args.index("--")
    parent, new = load(args[:cut]), load(args[cut + 1:])
    print("| kernel (parent instance) | vgpr | agpr | sgpr | spills v / s | LDS | private | instructions parent / new | stream | counted opcodes | "
          "arch vgpr | scratch | waves / SIMD | " + " / ".join(c for c, _ in CLASSES) + " |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    bad = 0
    seen = set()
    for name in sorted(new):
        pname = name
        for pat, rep in RENAMED:
            if re.match(pat, name):
                pname = re.sub(pat, rep, name)
        if pname not in parent:
            print(f"| {name} | new: no parent instance | | | | | | | | | | | | |")
            bad += 1
            continue
        seen.add(pname)
        (pm, pb), (nm, nb) = parent[pname], new[name]
        both = lambda k: str(nm[k]) if nm[k] == pm[k] else f"**{pm[k]} -> {nm[k]}**"
        same = pb == nb
        diff = {op: (opcounts(pb)[op], opcounts(nb)[op]) for op in set(opcounts(pb)) | set(opcounts(nb))
                if opcounts(pb)[op] != opcounts(nb)[op]}
        cp, cn = classes(pb), classes(nb)
        if pm != nm or diff:
            bad += 1
        ni = lambda b: sum(1 for ln in b if not ln.endswith(":"))
        label = pname if pname == name else f"{pname} <- {name}"
        print(f"| {label} | {both('vgpr_count')} | {both('agpr_count')} | {both('sgpr_count')} | {both('vgpr_spill_count')} / "
              f"{both('sgpr_spill_count')} | {both('group_segment_fixed_size')} | {both('private_segment_fixed_size')} | "
              f"{ni(pb)} / {ni(nb)} | {'identical' if same else 'differs'} | "
              f"{'equal' if not diff else ', '.join(f'{op} {a} -> {b}' for op, (a, b) in sorted(diff.items()))} | "
              f"{both('NumVgprs')} | {both('ScratchSize')} | {both('Occupancy')} | "
              f"{' / '.join(str(b) if a == b else f'**{a} -> {b}**' for a, b in zip(cp, cn))} |")
    for name in sorted(set(parent) - seen):
        print(f"| {name} | parent only | | | | | | | | | | | | |")
        bad += 1
    print(f"\n{len(new)} kernels, {len(parent)} in the parent; rows with a resource or counted-opcode difference or without a "
          f"partner: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
