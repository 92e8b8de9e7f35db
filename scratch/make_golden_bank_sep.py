"""Fixture of the per-video frame masks a SEP / svsq batch carries (`pad_frm_mask`), from the REFERENCE loader's own
`get_frm_mask` and padding arithmetic (code/dat_loader_simple.py:405-416, :237-255). Runs where the reference tree is present
(`oracle.ref_import.available()`); writes tests/golden/bank_sep_frm_mask.npz - inputs and expected output, a few KB.

    python scratch/make_golden_bank_sep.py

Videos: 0 without boxes, 1 with G boxes, 2 / 3 with padded proposals, 4 without any proposal, 5 full. The last real proposal
of every video is an included one (pnt = 1), which is how `FeatureBank` finds the number of real proposals; proposals in
front of it may be excluded (pnt = 0) and still count as real."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

synth = importlib.import_module("vognet-pytorch_amd.synth")
V, NPPF, G = 6, 5, 6
OUT = os.path.join(ROOT, "tests", "golden", "bank_sep_frm_mask.npz")


def inputs():
    NPv = synth.NFRM0 * NPPF
    it = synth.make_items(V, 1, NPPF, prop_dim=8, seg_dim=8, n_gt=G, seed=31)
    rng = np.random.default_rng(32)
    props = np.ascontiguousarray(it["pad_proposals"][:, 0])
    gt = np.ascontiguousarray(it["pad_gt_bboxs"][:, 0])
    num_box = np.array([0, G, 3, 5, 2, 4], np.int64)
    num_props = np.array([NPv, NPv, 37, 12, 0, NPv], np.int64)
    pnt = (rng.uniform(size=(V, NPv)) < 0.8).astype(np.uint8)
    for v in range(V):
        n = int(num_props[v])
        props[v, n:] = 0                                   # pad_words_with_vocab(..., defm=[[0] * 7])
        pnt[v, n:] = 0
        if n:
            pnt[v, n - 1] = 1
    return {"pad_proposals": props, "pad_pnt_mask": pnt, "pad_gt_bboxs": gt, "num_box": num_box, "num_props": num_props}


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not present (oracle.ref_import.available()): the committed fixture stays as it is")
    ref_import.install_stubs()
    if "h5py" not in sys.modules:
        sys.modules["h5py"] = types.ModuleType("h5py")
    import dat_loader_simple as ref  # noqa: the reference module
    ds = ref.Anet_SRL.__new__(ref.Anet_SRL)
    x = inputs()
    NPv = x["pad_proposals"].shape[1]
    out = np.zeros((V, NPv, G), np.uint8)
    for v in range(V):
        n, nb = int(x["num_props"][v]), int(x["num_box"][v])
        m = np.ones((NPv, G))                              # pad_frm_mask = np.ones((max_proposals, max_gt_box))
        m[:n, :nb] = ds.get_frm_mask(x["pad_proposals"][v, :n, 4], x["pad_gt_bboxs"][v, :nb, 4])
        out[v] = m.astype(np.uint8)
    np.savez_compressed(OUT, pad_frm_mask=out, **x)
    print(OUT, os.path.getsize(OUT), "bytes", {v: int((out[v] == 0).sum()) for v in range(V)})


if __name__ == "__main__":
    main()
