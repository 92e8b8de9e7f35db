"""Host side of the in-place weight refresh: the three new ABI entries are declared on both sides, cfg.hip.weight_refresh is
checked, and the shared index maps (csrc/wpack_dev.h: what the host packers and the device pack kernels both call) are
bijections that place every element where the host packers place it. No GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("vognet-pytorch_amd.lib")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")

FRAG16, FRAG32, LSTM = 1, 2, 3


def test_header_and_binding_declare_the_new_entries():
    src = open(os.path.join(ROOT, "include", "vog_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for n in ("vog_ctx_num_images", "vog_ctx_image_info", "vog_ctx_refresh_device"):
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert n in L.SYMBOLS and hasattr(lib, n), n
    assert "vog_weight_src" in src and "vog_image_info" in src
    assert [f[0] for f in L.WeightSrc._fields_] == ["name", "dev", "numel"]
    # a context that is not finalized has no table and refuses a refresh before anything else
    assert lib.vog_ctx_num_images(None) == -1
    assert lib.vog_ctx_refresh_device(None, None, 0, None) != 0


def test_weight_refresh_option_is_validated():
    cfg = ec.get_default_cfg()
    assert cfg.hip.weight_refresh == "host"
    for ok in ("host", "device"):
        cfg.hip.weight_refresh = ok
        ec.check_hip_options(cfg)
        assert ec.parse_weight_refresh(cfg.hip) == ok
    for bad in ("gpu", "", "Device", 1, None):
        cfg.hip.weight_refresh = bad
        with pytest.raises(ValueError, match="weight_refresh"):
            ec.check_hip_options(cfg)
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, {"hip.weight_refresh": "device"})
    assert cfg.hip.weight_refresh == "device"


def _index_map(layout, N, K, total):
    out = np.full(total, -1, np.int64)
    L.check(L.load().vog_wpack_index_map(layout, N, K, out.ctypes.data), "vog_wpack_index_map")
    return out


def _own_index_matrix(rows, K):
    """entries = their own linear index, all <= 2048: exact in f16 (and in fp32)"""
    assert rows * K <= 2049
    return np.arange(rows * K, dtype=np.float32).reshape(rows, K)


@pytest.mark.parametrize("N,K", [(16, 32), (32, 64), (48, 32)])
def test_fragment_maps_are_bijections_and_match_the_host_packers(N, K):
    lib = L.load()
    w = _own_index_matrix(N, K)
    todo = [(FRAG16, lib.vog_pack_w_frag)]
    if N % 32 == 0:                               # (the 32x16 order takes row blocks of 32)
        todo.append((FRAG32, lib.vog_pack_w_frag32))
    for layout, packer in todo:
        m = _index_map(layout, N, K, N * K)
        assert np.array_equal(np.sort(m), np.arange(N * K)), layout
        dst = np.zeros(N * K, np.float16)
        L.check(packer(w.ctypes.data, K, N, K, dst.ctypes.data, L.VOG_F16), "pack")
        assert np.array_equal(dst.astype(np.int64), m), layout      # the value read back IS the source position
    if N % 32:
        assert lib.vog_wpack_index_map(FRAG32, N, K, np.zeros(N * K, np.int64).ctypes.data) != 0


def test_lstm_map_is_a_bijection_and_matches_the_host_packer():
    lib = L.load()
    R, K = 4, 32                                  # the smallest legal pack: R % 4, K % 32
    w = _own_index_matrix(8 * R, K)               # [W_fwd ; W_bwd]
    m = _index_map(LSTM, R, K, 8 * R * K)
    assert np.array_equal(np.sort(m), np.arange(8 * R * K))
    dst = np.zeros(8 * R * K, np.float16)
    L.check(lib.vog_lstm_pack_w(w[:4 * R].ctypes.data, w[4 * R:].ctypes.data, dst.ctypes.data, R, K, L.VOG_F16), "pack")
    assert np.array_equal(dst.astype(np.int64), m)
    assert lib.vog_wpack_index_map(LSTM, 6, K, m.ctypes.data) != 0 and lib.vog_wpack_index_map(LSTM, R, 48, m.ctypes.data) != 0
    assert lib.vog_wpack_index_map(0, R, K, m.ctypes.data) != 0 and lib.vog_wpack_index_map(FRAG16, 16, 32, None) != 0
