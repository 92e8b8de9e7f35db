"""Host side of the mixed-precision training mode (no GPU): the library's per-thread "amp" switch and "f32_products"
counter (include/vog_hip.h, vog_train_set_int), `cfg.hip.train_amp` through the command line and the config checks, and
the argument checks of FP32Trainer / Learner that run before any device work."""
import ctypes
import importlib
import threading

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
trn = importlib.import_module("vognet-pytorch_amd.train")


def _get(lib, name):
    v = ctypes.c_int32(-1)
    assert lib.vog_train_get_int(name, ctypes.byref(v)) == 0
    return v.value


def test_amp_switch_reads_back_and_is_per_thread():
    lib = L.load()
    try:
        assert lib.vog_train_set_int(b"amp", 1) == 0 and _get(lib, b"amp") == 1
        seen = {}

        def other():
            seen["before"] = _get(lib, b"amp")
            lib.vog_train_set_int(b"amp", 2)
            seen["after"] = _get(lib, b"amp")

        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert seen == {"before": 0, "after": 2}
        assert _get(lib, b"amp") == 1                 # the other thread's write did not reach this one
        assert lib.vog_train_set_int(b"amp", 2) == 0 and _get(lib, b"amp") == 2
    finally:
        assert lib.vog_train_set_int(b"amp", 0) == 0
    assert _get(lib, b"amp") == 0


@pytest.mark.parametrize("bad", [-1, 3, 16])
def test_amp_switch_rejects_values_outside_0_to_2(bad):
    lib = L.load()
    assert lib.vog_train_set_int(b"amp", bad) != 0
    assert _get(lib, b"amp") == 0


def test_f32_product_counter_reads_and_resets():
    lib = L.load()
    assert lib.vog_train_set_int(b"f32_products", 0) == 0 and _get(lib, b"f32_products") == 0
    assert lib.vog_train_set_int(b"f32_products", 5) != 0    # a counter: only a reset to 0 is accepted


def test_train_amp_config_key_and_command_line():
    cfg = ec.get_default_cfg()
    assert cfg.hip.train_amp == ""
    assert tu.train_amp(cfg) is None
    uid, kw = main_mod.parse_argv(["run1", "--hip.train_amp=bf16"])
    assert uid == "run1" and kw == {"hip.train_amp": "bf16"}
    ec.update_from_dict(cfg, kw)
    assert cfg.hip.train_amp == "bf16" and tu.train_amp(cfg) == "bf16"


def test_train_amp_f16_and_unknown_modes_are_refused():
    cfg = ec.get_default_cfg()
    cfg.hip.train_amp = "f16"
    with pytest.raises(ValueError, match="GradScaler"):
        tu.train_amp(cfg)
    cfg.hip.train_amp = "fp8"
    with pytest.raises(ValueError):
        tu.train_amp(cfg)
    # a reference yacs config has no `hip` section: fp32
    del cfg["hip"]
    assert tu.train_amp(cfg) is None


def test_trainer_refuses_amp_with_bf16_gemm_and_unknown_modes():
    cfg = ec.get_default_cfg()
    with pytest.raises(ValueError, match="bf16_gemm"):
        trn.FP32Trainer(cfg, {}, {}, None, amp="bf16", bf16_gemm=True)
    with pytest.raises(ValueError, match="amp"):
        trn.FP32Trainer(cfg, {}, {}, None, amp="fp16")
