"""ms per cfg-2 full training step of this tree against the parent commit's build, fp32 and amp bf16, timed alternately in one
process (the method of scratch/time_finetune.py --parent: the parent's package is imported under another name with its own
libvog_hip.so next to it).

    python scratch/time_train_dedupe.py PARENT_DIR OUT.json [--rounds N] [--steps K]

Condition per mode: the new median lies within the parent's own spread (max - min of its rounds) of the parent's median."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_finetune as tf  # noqa: E402

from oracle import cases  # noqa: E402
from tests.gpu_util import comm_for  # noqa: E402
import numpy as np  # noqa: E402


def main():
    parent_dir, out = sys.argv[1], sys.argv[2]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 7
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    torch.cuda.set_device(0)
    ptrn, psel = tf.load_parent(parent_dir)
    assert os.path.dirname(ptrn.L.LIB_PATH) != os.path.dirname(tf.L.LIB_PATH), (ptrn.L.LIB_PATH, tf.L.LIB_PATH)
    cfg, sd, batch, c = cases.build(tf.CFG2)
    tg = tf.synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    fns = {}
    for tag, amp in (("fp32", None), ("amp_bf16", "bf16")):
        for who, trn, sel in (("parent", ptrn, psel), ("new", tf.trn, tf.sel_mod)):
            loss_fn = sel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))
            t = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp)
            fns[f"{tag}/{who}"] = lambda t=t: t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                       # parent and new alternate: drift hits both alike
        for m, fn in fns.items():
            res[m].append(tf.timed(fn, steps))
    modes = {}
    for tag in ("fp32", "amp_bf16"):
        p, n = tf.stats(res[f"{tag}/parent"]), tf.stats(res[f"{tag}/new"])
        modes[tag] = {"parent": p, "new": n, "new_minus_parent_median_ms": n["median"] - p["median"],
                      "within_parent_spread": bool(abs(n["median"] - p["median"]) <= p["spread"]),
                      "not_slower_by_more_than_parent_spread": bool(n["median"] - p["median"] <= p["spread"])}
    losses = {m: float(fn()["loss"]) for m, fn in fns.items()}
    summary = {"case": tf.CFG2, "rounds": rounds, "steps_per_round": steps, "device": torch.cuda.get_device_name(0),
               "libraries": {"parent": ptrn.L.LIB_PATH.replace(os.path.dirname(HERE), "."), "new": tf.L.LIB_PATH.replace(os.path.dirname(HERE), ".")},
               "step_ms": modes, "loss_after": losses}
    print(json.dumps({t: {"parent": m["parent"]["median"], "parent_spread": m["parent"]["spread"], "new": m["new"]["median"],
                          "within": m["within_parent_spread"]} for t, m in modes.items()}))
    print(json.dumps(losses))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
