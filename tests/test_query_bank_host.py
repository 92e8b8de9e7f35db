"""CPU: the host side of the query bank - the new C structs against gcc's layout, the new exports, the argument errors of
vog_gather_rows that are raised before anything touches a device, and the host logic of `QueryBank` (concatenation checks,
the host metadata columns, the index checks)."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("vognet-pytorch_amd.lib")
dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
main_dist = importlib.import_module("vognet-pytorch_amd.main_dist")

NEW_EXPORTS = ("vog_gather_rows", "vog_graph_capture_desc")


def test_query_bank_structs_match_the_c_header(tmp_path):
    """sizeof and the offset of the last member of the three new structs as gcc lays them out, against the ctypes mirrors;
    the key array's offset and stride, and the two limits."""
    pairs = {"vog_gather_key": L.GatherKey, "vog_gather_args": L.GatherArgs, "vog_fed_desc": L.FedDesc}
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vog_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append(f'  printf("{cname} %zu %zu\\n", sizeof({cname}), offsetof({cname}, {cls._fields_[-1][0]}));')
    src.append('  printf("keys %zu %zu %zu\\n", offsetof(vog_gather_args, keys), offsetof(vog_gather_args, Q), offsetof(vog_gather_args, n_keys));')
    src.append('  printf("desc %zu %zu %zu\\n", offsetof(vog_fed_desc, gather), offsetof(vog_fed_desc, bank_args), offsetof(vog_fed_desc, nseg));')
    src.append('  printf("limits %d %d\\n", VOG_MAX_GATHER_KEYS, VOG_MAX_COPY_SEGS);')
    src += ['  return 0;', '}']
    (tmp_path / "abi.c").write_text("\n".join(src))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")], check=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line in out[:3]:
        cname, size, off = line.split()
        cls = pairs[cname]
        assert C.sizeof(cls) == int(size), (cname, C.sizeof(cls), size)
        assert getattr(cls, cls._fields_[-1][0]).offset == int(off), (cname, off)
    assert [int(x) for x in out[3].split()[1:]] == [L.GatherArgs.keys.offset, L.GatherArgs.Q.offset, L.GatherArgs.n_keys.offset]
    assert [int(x) for x in out[4].split()[1:]] == [L.FedDesc.gather.offset, L.FedDesc.bank_args.offset, L.FedDesc.nseg.offset]
    assert [int(x) for x in out[5].split()[1:]] == [L.MAX_GATHER_KEYS, L.MAX_COPY_SEGS] == [32, 24]
    assert L.GatherArgs.keys.size == 32 * C.sizeof(L.GatherKey)


def test_query_bank_exports_are_built_and_declared():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vog_hip.h")).read(), flags=re.S)
    for n in NEW_EXPORTS:
        assert hasattr(lib, n), f"libvog_hip.so does not export {n}"
        assert n in L.SYMBOLS and re.search(rf"\bint\s+{n}\s*\(", hdr), n
    assert lib.vog_graph_capture_desc(None, None, None) != 0 and b"bad argument" in (lib.vog_last_error() or b"")


def _good_args(buf, n_keys=1, B=2, Q=4, row_bytes=8):
    """A well-formed argument block over host memory (never launched: every call below fails its argument check)."""
    a = L.GatherArgs()
    p = buf.ctypes.data
    a.index, a.B, a.Q, a.n_keys = p, B, Q, n_keys
    for i in range(min(max(n_keys, 1), L.MAX_GATHER_KEYS)):
        a.keys[i].table, a.keys[i].dst, a.keys[i].row_bytes, a.keys[i].per_batch = p + 64, p + 128, row_bytes, 0
    return a


@pytest.mark.parametrize("what", ["n_keys0", "n_keys33", "B0", "Q0", "row_bytes0", "null_table", "null_dst", "null_index", "null_args"])
def test_gather_rows_argument_errors_touch_no_device(what):
    """Every argument error returns through the check in front of the first HIP call: non-zero with a message, on a machine
    without a device and with a null stream."""
    lib = L.load()
    buf = np.zeros(64, np.int64)
    a = _good_args(buf)
    if what == "n_keys0":
        a.n_keys = 0
    elif what == "n_keys33":
        a.n_keys = 33
    elif what == "B0":
        a.B = 0
    elif what == "Q0":
        a.Q = 0
    elif what == "row_bytes0":
        a.keys[0].row_bytes = 0
    elif what == "null_table":
        a.keys[0].table = None
    elif what == "null_dst":
        a.keys[0].dst = None
    elif what == "null_index":
        a.index = None
    rc = lib.vog_gather_rows(None if what == "null_args" else C.byref(a), None)
    assert rc != 0 and b"bad argument" in (lib.vog_last_error() or b""), what
    assert not buf.any()


def _host_qbank(Q, spec, host_keys):
    """A query bank with its tables on the host: `put`, `meta` and the index checks are plain host logic."""
    q = dls.QueryBank.__new__(dls.QueryBank)
    q.Q, q.device = Q, torch.device("cpu")
    q.spec = {k: dls._row_spec(v) for k, v in spec.items()}
    q.host_keys = tuple(host_keys)
    q.tab = {k: torch.zeros((Q,) + shp, dtype=dt) for k, (shp, dt) in q.spec.items()}
    q.host = {k: torch.zeros((Q,) + q.spec[k][0], dtype=q.spec[k][1]).numpy() for k in q.host_keys}
    return q


def _batches(sizes=(4, 4, 3)):
    out, r = [], 0
    for n in sizes:
        out.append({"srl_arg_words_ind": torch.arange(r * 6, (r + n) * 6, dtype=torch.int64).view(n, 2, 3),
                    "target_cmp": torch.arange(r, r + n, dtype=torch.int64) % 3,
                    "sent_idx": torch.arange(100 + r, 100 + r + n, dtype=torch.int64),
                    "permute": torch.stack([torch.roll(torch.arange(4), int(i)) for i in range(r, r + n)]).to(torch.int64)})
        r += n
    return out


def test_from_batches_refuses_mismatched_rows(monkeypatch):
    """The concatenation checks run before anything is allocated: a key whose row shape or dtype differs between batches, a
    key a batch lacks, and batch sizes that differ between keys are ValueErrors; the ragged last batch is fewer rows."""
    def fake_init(self, n_queries, spec, device=None, host_keys=None):
        q = _host_qbank(n_queries, {k: v for k, v in spec.items()}, host_keys)
        self.__dict__.update(q.__dict__)

    monkeypatch.setattr(dls.QueryBank, "__init__", fake_init)
    qb = dls.QueryBank.from_batches(_batches())
    assert qb.Q == 11 and qb.host_keys == ("sent_idx", "target_cmp", "permute")         # META_KEYS order, those present
    assert torch.equal(qb.tab["target_cmp"], torch.arange(11) % 3) and tuple(qb.tab["srl_arg_words_ind"].shape) == (11, 2, 3)
    assert qb.nbytes == 11 * (6 + 1 + 1 + 4) * 8 and qb.row_bytes("srl_arg_words_ind") == 48 and set(qb.keys) == set(_batches()[0])
    bad = _batches()
    bad[1]["srl_arg_words_ind"] = bad[1]["srl_arg_words_ind"].reshape(4, 3, 2)
    with pytest.raises(ValueError, match="srl_arg_words_ind"):
        dls.QueryBank.from_batches(bad)
    bad = _batches()
    bad[2]["target_cmp"] = bad[2]["target_cmp"].to(torch.int32)
    with pytest.raises(ValueError, match="target_cmp"):
        dls.QueryBank.from_batches(bad)
    bad = _batches()
    del bad[1]["permute"]
    with pytest.raises(ValueError, match="permute"):
        dls.QueryBank.from_batches(bad)
    bad = _batches()
    bad[0]["sent_idx"] = bad[0]["sent_idx"][:3]
    with pytest.raises(ValueError, match="sent_idx"):
        dls.QueryBank.from_batches(bad)
    with pytest.raises(ValueError, match="no batches"):
        dls.QueryBank.from_batches([])
    sub = dls.QueryBank.from_batches(_batches(), keys=["target_cmp", "permute"], host_keys=["permute"])
    assert set(sub.keys) == {"target_cmp", "permute"} and sub.host_keys == ("permute",)


def test_meta_put_and_index_checks():
    bts = _batches()
    full = {k: torch.cat([b[k] for b in bts]) for k in bts[0]}
    qb = _host_qbank(11, bts[0], ("sent_idx", "target_cmp", "permute"))
    qb.put(0, {k: v[:4] for k, v in full.items()})
    qb.put(4, {k: v[4:].numpy() for k, v in full.items()})
    for idx in (np.array([10, 0, 3, 3, 10, 7]), torch.tensor([2, 1, 0], dtype=torch.int32), [5], np.arange(11)[::-1]):
        rows = qb.meta(idx)
        i = np.asarray(idx).reshape(-1)
        assert set(rows) == {"sent_idx", "target_cmp", "permute"}
        for k in rows:
            assert np.array_equal(rows[k], full[k].numpy()[i]), k
    assert qb.meta(np.array([3, 3]))["permute"].shape == (2, 4)
    for idx in ([11], [-1, 0]):
        with pytest.raises(ValueError, match="outside"):
            qb.meta(idx)
        with pytest.raises(ValueError, match="outside"):
            qb._index(torch.tensor(idx, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        qb._index(torch.zeros(4))
    with pytest.raises(ValueError, match="int32"):
        qb._index(torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows 9 .. 12"):
        qb.put(9, {k: v[:3] for k, v in full.items()})
    with pytest.raises(ValueError, match="target_cmp"):
        qb.put(0, {"target_cmp": full["target_cmp"][:2].to(torch.int32)})
    with pytest.raises(ValueError, match="none of the items"):
        qb.put(0, {"other": full["target_cmp"]})
    qb._bad = torch.zeros(16, dtype=torch.int32)
    qb.check()
    qb._bad[0] = 1
    with pytest.raises(L.VogError, match="outside"):
        qb.check()
    qb.check()                                                 # reported once


def test_config_and_cli():
    cfg = ec.get_default_cfg()
    assert cfg.hip.query_bank is False and cfg.hip.val_graph is False
    ec.update_from_dict(cfg, {"hip.query_bank": "True"})
    assert cfg.hip.query_bank is True
    uid, kw = main_dist.parse_argv(["exp1", "--feature_bank=f16", "--query_bank=True", "--only_val"])
    assert kw["query_bank"] == "True" and kw["feature_bank"] == "f16"
    with pytest.raises(SystemExit, match="feature_bank"):
        main_dist.main_dist("exp1", query_bank="True", only_val="True")
