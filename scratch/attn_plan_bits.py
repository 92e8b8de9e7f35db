"""Bytes of the forward's outputs of this tree against another tree (attn_plan: the parent commit's checkout with its library
built), one child process per tree in the manner of bits_vs_parent.py - a tree, not only a library, because lib.load() types
exports a parent build does not have.

    python scratch/attn_plan_bits.py PARENT_TREE OUT.json
    python scratch/attn_plan_bits.py --child TREE

Each child runs, eagerly and from a graph slot, the forward of CASES on the precision plan `auto` picks (f16 kernels; hi + lo
operands for the sharp checkpoint) and prints the SHA-256 of every output tensor."""
import hashlib
import json
import os
import subprocess
import sys

CASES = ["small/vog_spat", "full/cfg2_vog_spat_gt5_bs4", "full/cfg4_vog_spat_p100_bs4", "full/cfg2_sharp16"]


def child(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from tests.gpu_util import build_engine
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    out = {}
    for name in CASES:
        eng, cfg, sd, batch, c, dev = build_engine(name)
        res = eng.forward(dev)
        torch.cuda.synchronize()
        out[name] = {"plan": eng.plan, **{"eager/" + k: sha(v) for k, v in sorted(res.items()) if torch.is_tensor(v)}}
        slot = eng.make_slot(dev, graph=True)
        slot.launch()
        torch.cuda.synchronize()
        res = slot.launch()
        torch.cuda.synchronize()
        out[name].update({"graph/" + k: sha(v) for k, v in sorted(res.items()) if torch.is_tensor(v)})
    print("BITS " + json.dumps(out))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for tag, tree in (("parent", os.path.abspath(sys.argv[1])), ("new", here)):
        env = {k: v for k, v in os.environ.items() if k != "VOG_HIP_LIB"}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], env=env, cwd=tree, capture_output=True, text=True,
                           timeout=600)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:])
            raise SystemExit(f"{tag} child ended with {r.returncode}")
        got[tag] = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("BITS ")][-1][5:])
    report = {}
    for name in CASES:
        a, b = got["parent"][name], got["new"][name]
        report[name] = {"plan": b["plan"], "tensors": len(b) - 1, "differing": sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))}
    report["byte_equal"] = not any(report[n]["differing"] for n in CASES)
    print(json.dumps(report, indent=1))
    with open(sys.argv[2], "w") as f:
        json.dump(report, f, indent=1)
    return 0 if report["byte_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
