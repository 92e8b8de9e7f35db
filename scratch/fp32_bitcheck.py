"""fp32 training outputs of one build, for a bitwise comparison of two builds (e.g. a change against its parent):

    python scratch/fp32_bitcheck.py dump ROOT OUT.pt     # ROOT: the tree whose package (and libvog_hip.so) runs
    python scratch/fp32_bitcheck.py compare A.pt B.pt

dump: FP32Trainer.gradients (eval and train-mode dropout) and autograd's p.grad after loss.backward(), plus the losses of
three FP32Trainer steps, on a few cases - all outside any mixed-precision mode. compare: every tensor bit for bit."""
import importlib
import os
import sys

import numpy as np
import torch

CASES = ["small/vog_spat", "small/vog_sep_cmpmsk", "full/cfg2_vog_spat_gt5_bs4", "full/cfg5_vog_svsq_gt5_bs16"]


def dump(root, out):
    sys.path.insert(0, os.path.abspath(root))
    from oracle import cases
    from tests.gpu_util import comm_for
    trn = importlib.import_module("vognet-pytorch_amd.train")
    synth = importlib.import_module("vognet-pytorch_amd.synth")
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    torch.cuda.set_device(0)
    res = {}
    for name in CASES:
        cfg, sd, batch, c = cases.build(name)
        sel = sel_mod.get_mdl_loss_eval(cfg)
        comm = comm_for(c)
        tg = synth.make_targets(batch, cfg.ds.conc_type, c["nppf0"], seed=c["dseed"])
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**batch, **tg}.items()}
        sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
        loss_fn = sel["loss"](cfg, comm)
        for drop in (False, True):
            tr = trn.FP32Trainer(cfg, comm, sdt, loss_fn, lr=1e-4, dropout=drop, dropout_seed=3)
            ld, g = tr.gradients(dev)
            res[f"{name}|trainer|drop={drop}|loss"] = ld["loss"].detach().cpu().reshape(1)
            res.update({f"{name}|trainer|drop={drop}|{k}": v.detach().cpu() for k, v in g.items()})
        mdl = sel["mdl"](cfg=cfg, comm=comm)
        mdl.load_state_dict(sdt)
        mdl = mdl.cuda().eval().requires_grad_(True)
        loss = loss_fn(mdl(dev), dev)["loss"]
        loss.backward()
        res[f"{name}|autograd|loss"] = loss.detach().cpu().reshape(1)
        res.update({f"{name}|autograd|{n}": p.grad.detach().cpu() for n, p in mdl.named_parameters() if p.grad is not None})
        tr = trn.FP32Trainer(cfg, comm, sdt, loss_fn, lr=1e-4)
        res[f"{name}|steps"] = torch.tensor([float(tr.step(dev)["loss"]) for _ in range(3)])
        res.update({f"{name}|after_steps|{k}": v.cpu() for k, v in tr.state_dict().items()})
    torch.save(res, out)
    print(f"{len(res)} tensors -> {out}")


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    assert set(a) == set(b), sorted(set(a) ^ set(b))[:10]
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    print(f"{len(a)} tensors, {len(bad)} differ" + (f": {bad[:10]}" if bad else " (bit-identical)"))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
