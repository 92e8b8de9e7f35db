"""Host side of `cfg.hip.val_graph` (no GPU): the config key and its CLI form, the refusal of `batch_requests > 1`, the silent
fall-back of a CPU evaluator, and the SEP frame-mask rule of `FeatureBank` restated in numpy against the fixture made with the
reference loader's `get_frm_mask` (scratch/make_golden_bank_sep.py -> tests/golden/bank_sep_frm_mask.npz)."""
import importlib
import os

import numpy as np
import pytest
import torch

ec = importlib.import_module("vognet-pytorch_amd.extended_config")
E = importlib.import_module("vognet-pytorch_amd.eval_vsrl_corr")
L = importlib.import_module("vognet-pytorch_amd.lib")
main_dist = importlib.import_module("vognet-pytorch_amd.main_dist")

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bank_sep_frm_mask.npz")


def sep_frm_mask(props, pnt, gt, num_box):
    """The rule of vog_assemble_from_bank for one video: props [NPv, 7], pnt [NPv], gt [G, 5] -> [NPv, G] bytes. The real
    proposals end behind the last nonzero byte of `pnt`; byte = 1 except where a real proposal and a gt box g < num_box share
    their frame."""
    NPv, G = props.shape[0], gt.shape[0]
    nz = np.nonzero(pnt)[0]
    n = int(nz[-1]) + 1 if len(nz) else 0
    nb = int(min(max(num_box, 0), G))
    out = np.ones((NPv, G), np.uint8)
    out[:n, :nb] = (props[:n, 4][:, None] != gt[:nb, 4][None, :]).astype(np.uint8)
    return out


def test_default_is_off_and_the_cli_sets_it():
    cfg = ec.get_default_cfg()
    assert cfg.hip.val_graph is False
    uid, kw = main_dist.parse_argv(["e1", "--hip.val_graph=True", "--only_val"])
    ec.update_from_dict(cfg, kw)
    assert cfg.hip.val_graph is True and cfg.only_val is True
    with pytest.raises(AssertionError):
        ec.update_from_dict(cfg, {"hip.val_graph": "yes"})


def test_val_graph_with_batch_requests_is_refused(tmp_path):
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"hip.val_graph": True, "hip.batch_requests": 2})
    evl = E.EvaluatorSPAT(cfg, {"num_prop_per_frm": 5}, "cpu")
    with pytest.raises(ValueError, match="batch_requests"):
        evl(torch.nn.Identity(), None, [], "valid", pred_path=tmp_path)
    assert not any(tmp_path.iterdir())


def test_cpu_evaluator_keeps_the_existing_loop(tmp_path):
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"hip.val_graph": True})
    evl = E.EvaluatorSPAT(cfg, {"num_prop_per_frm": 5}, "cpu")
    evl(torch.nn.Identity(), None, [], "valid", pred_path=tmp_path)
    assert evl.val_path == "eager"


def test_ctypes_mirrors_of_the_new_structs(tmp_path):
    """sizeof / last-member offset of vog_val_log_args, vog_val_epilogue and vog_gmetric_args (which gained `log`) as gcc lays
    them out."""
    import ctypes as C
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"vog_val_log_args": L.ValLogArgs, "vog_val_epilogue": L.ValEpilogue, "vog_gmetric_args": L.GMetricArgs}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vog_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append(f'  printf("{cname} %zu %zu\\n", sizeof({cname}), offsetof({cname}, {cls._fields_[-1][0]}));')
    src += ['  return 0;', '}']
    (tmp_path / "abi.c").write_text("\n".join(src))
    subprocess.run([shutil.which("gcc"), "-I", os.path.join(root, "include"), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")], check=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        cname, size, off = line.split()
        cls = pairs[cname]
        assert C.sizeof(cls) == int(size) and getattr(cls, cls._fields_[-1][0]).offset == int(off), cname


def test_sep_mask_rule_equals_the_reference_fixture():
    g = np.load(GOLD)
    V = g["pad_proposals"].shape[0]
    assert (g["num_box"] == 0).any() and (g["num_box"] == g["pad_gt_bboxs"].shape[1]).any()        # no boxes / G boxes
    assert (g["num_props"] < g["pad_proposals"].shape[1]).any() and (g["num_props"] == 0).any()    # padded proposals / none
    zeros = 0
    for v in range(V):
        nz = np.nonzero(g["pad_pnt_mask"][v])[0]
        assert (int(nz[-1]) + 1 if len(nz) else 0) == int(g["num_props"][v])      # the fixture's count is what the rule finds
        got = sep_frm_mask(g["pad_proposals"][v], g["pad_pnt_mask"][v], g["pad_gt_bboxs"][v], int(g["num_box"][v]))
        assert np.array_equal(got, g["pad_frm_mask"][v]), v
        zeros += int((got == 0).sum())
    assert zeros > 0
    # an excluded proposal in front of the last included one still counts as real
    v = int(np.argmax(g["num_props"] == g["pad_proposals"].shape[1]))
    assert (g["pad_pnt_mask"][v] == 0).any()


def test_synthetic_index_loader_carries_the_sep_keys():
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"ds.conc_type": "svsq"})
    comm = {"vocab_size": 200, "detect_size": 431, "itod": {}, "wtoi": {"UNK": 1}, "num_prop_per_frm": ec.num_prop_per_frm(cfg)}
    dl = main_dist.synthetic_index_loader(cfg, comm, 3, 0, 1, 16)
    bs = int(cfg.train.bsv)
    assert tuple(dl[0]["verb_cmp"].shape) == (bs, 1) and tuple(dl[0]["verb_cross_cmp_msk"].shape) == (bs, 1, 1)
    assert dl[0]["vid_index"].dtype == torch.int32 and int(dl[-1]["verb_cmp"].shape[0]) == bs - 1
