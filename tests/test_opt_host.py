"""Host side of the fused optimiser step (no GPU): the config keys `hip.train_loss_scale` / `hip.train_clip_norm` through the
command line and the config checks, the argument checks of FP32Trainer that run before any device work, and those of
vog_opt_step_f32 (include/vog_hip.h), which run before any launch - so pointers that are never dereferenced do here."""
import ctypes as C
import importlib

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
trn = importlib.import_module("vognet-pytorch_amd.train")


def test_config_keys_defaults_and_command_line():
    cfg = ec.get_default_cfg()
    assert cfg.hip.train_loss_scale == "" and cfg.hip.train_clip_norm == 0.0
    assert tu.train_loss_scale(cfg) is None and tu.train_clip_norm(cfg) is None
    uid, kw = main_mod.parse_argv(["run1", "--hip.train_loss_scale=dynamic", "--hip.train_clip_norm=1.0"])
    assert uid == "run1" and kw == {"hip.train_loss_scale": "dynamic", "hip.train_clip_norm": "1.0"}
    ec.update_from_dict(cfg, kw)
    assert cfg.hip.train_loss_scale == "dynamic" and cfg.hip.train_clip_norm == 1.0
    assert tu.train_loss_scale(cfg) == "dynamic" and tu.train_clip_norm(cfg) == 1.0
    # a number for the text key stays text; an integer for the float key becomes a float
    _, kw = main_mod.parse_argv(["run1", "--hip.train_loss_scale=1024", "--hip.train_clip_norm=2"])
    ec.update_from_dict(cfg, kw)
    assert cfg.hip.train_loss_scale == "1024" and cfg.hip.train_clip_norm == 2.0
    assert tu.train_loss_scale(cfg) == 1024.0 and tu.train_clip_norm(cfg) == 2.0
    with pytest.raises(AssertionError):
        ec.update_from_dict(cfg, {"hip.train_clip_norm": "big"})
    # every other text key still refuses a number, as the reference does
    with pytest.raises(AssertionError, match="type mismatch"):
        ec.update_from_dict(cfg, {"hip.tx_dtype": "123"})
    with pytest.raises(AssertionError, match="type mismatch"):
        ec.update_from_dict(cfg, {"hip.train_amp": "16"})


def test_train_amp_f16_needs_a_loss_scale():
    cfg = ec.get_default_cfg()
    cfg.hip.train_amp = "f16"
    with pytest.raises(ValueError, match="GradScaler") as e:
        tu.train_amp(cfg)
    assert "train_loss_scale" in str(e.value)
    for s in ("dynamic", "1024"):
        cfg.hip.train_loss_scale = s
        assert tu.train_amp(cfg) == "f16"
    cfg.hip.train_amp = "bf16"
    assert tu.train_amp(cfg) == "bf16"
    cfg.hip.train_amp = "fp8"
    with pytest.raises(ValueError):
        tu.train_amp(cfg)
    del cfg["hip"]                                     # a reference yacs config: fp32, no scaling, no clipping
    assert tu.train_amp(cfg) is None and tu.train_loss_scale(cfg) is None and tu.train_clip_norm(cfg) is None


@pytest.mark.parametrize("bad", ["fast", "-3", "0", "inf", "nan"])
def test_malformed_loss_scale_is_refused(bad):
    cfg = ec.get_default_cfg()
    cfg.hip.train_loss_scale = bad
    with pytest.raises(ValueError, match="train_loss_scale"):
        tu.train_loss_scale(cfg)
    cfg.hip.train_amp = "f16"
    with pytest.raises(ValueError):
        tu.train_amp(cfg)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_clip_norm_is_refused(bad):
    cfg = ec.get_default_cfg()
    cfg.hip.train_clip_norm = bad
    with pytest.raises(ValueError, match="train_clip_norm"):
        tu.train_clip_norm(cfg)


def test_trainer_refuses_bad_loss_scale_and_clip_norm_before_the_gpu():
    cfg = ec.get_default_cfg()
    for bad in ("fast", "-3", -3, 0, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="loss_scale"):
            trn.FP32Trainer(cfg, {}, {}, None, loss_scale=bad)
    for bad in (-1.0, 0.0, float("nan"), float("inf"), "1.0", True):
        with pytest.raises(ValueError, match="clip_norm"):
            trn.FP32Trainer(cfg, {}, {}, None, clip_norm=bad)
    for kw in ({"growth_interval": -1}, {"growth_interval": 2.5}, {"growth_factor": 0.5}, {"backoff_factor": 0.0},
               {"backoff_factor": 1.5}):
        with pytest.raises(ValueError, match="growth|backoff"):
            trn.FP32Trainer(cfg, {}, {}, None, loss_scale="dynamic", **kw)
    assert trn.parse_loss_scale(None) is None and trn.parse_loss_scale("dynamic") == 2.0 ** 16
    assert trn.parse_loss_scale("1024") == 1024.0 and trn.parse_loss_scale(8) == 8.0
    assert trn.parse_clip_norm(None) is None and trn.parse_clip_norm(1) == 1.0


# ---------------------------------------------------------------- vog_opt_step_f32: every argument fault, before any launch
FAKE = 0x10000          # never dereferenced: a faulty call returns before it touches the device


def _args(n_tensors=2, mode_b=False, **over):
    arr = (L.OptTensor * max(n_tensors, 1))()
    for i in range(max(n_tensors, 1)):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, 100
    a = L.OptArgs()
    a.tensors, a.n_tensors = arr, n_tensors
    a.lr, a.beta1, a.beta2, a.eps, a.step = 1e-3, 0.9, 0.99, 1e-8, 1
    if mode_b:
        a.state, a.scratch = FAKE + 0x4000, FAKE + 0x5000
        a.scratch_bytes = int(L.load().vog_opt_scratch_bytes(n_tensors, 100 * n_tensors))
        a.growth_factor, a.backoff_factor, a.growth_interval = 2.0, 0.5, 2000
    for k, v in over.items():
        setattr(a, k, v)
    return a, arr


def _tensor_fault(field, value):
    def make(mode_b):
        a, arr = _args(mode_b=mode_b)
        setattr(arr[1], field, value)
        return a, arr
    return make


FAULTS = {
    "p NULL": _tensor_fault("p", None), "g NULL": _tensor_fault("g", None), "m NULL": _tensor_fault("m", None),
    "v NULL": _tensor_fault("v", None), "n = 0": _tensor_fault("n", 0), "n < 0": _tensor_fault("n", -5),
    "tensors NULL": lambda b: _args(mode_b=b, tensors=C.POINTER(L.OptTensor)()),
    "n_tensors = 0": lambda b: _args(mode_b=b, n_tensors=0), "n_tensors < 0": lambda b: _args(mode_b=b, n_tensors=-1),
    "beta1 = 1": lambda b: _args(mode_b=b, beta1=1.0), "beta1 < 0": lambda b: _args(mode_b=b, beta1=-0.1),
    "beta2 = 1": lambda b: _args(mode_b=b, beta2=1.0), "beta2 < 0": lambda b: _args(mode_b=b, beta2=-0.1),
}


@pytest.mark.parametrize("mode_b", [False, True])
@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_opt_step_refuses_argument_faults(fault, mode_b):
    lib = L.load()
    a, keep = FAULTS[fault](mode_b)
    assert lib.vog_opt_step_f32(C.byref(a), None) != 0
    assert lib.vog_last_error(), fault


def test_opt_step_mode_a_needs_a_step_count_and_mode_b_its_scratch():
    lib = L.load()
    for step in (0, -1):
        a, keep = _args(step=step)
        assert lib.vog_opt_step_f32(C.byref(a), None) != 0
        assert b"step" in lib.vog_last_error()
    a, keep = _args(mode_b=True)
    a.scratch_bytes -= 1
    assert lib.vog_opt_step_f32(C.byref(a), None) != 0
    assert b"scratch" in lib.vog_last_error()
    a, keep = _args(mode_b=True, scratch=None)
    assert lib.vog_opt_step_f32(C.byref(a), None) != 0
    assert b"scratch" in lib.vog_last_error()
    assert lib.vog_opt_step_f32(None, None) != 0
    assert lib.vog_opt_scale_grad_f32(None, 4, FAKE, None) != 0 and lib.vog_opt_scale_grad_f32(FAKE, 0, FAKE, None) != 0
    assert lib.vog_opt_scale_grad_f32(FAKE, 4, None, None) != 0


def test_opt_scratch_bytes_is_positive_and_monotone():
    lib = L.load()
    counts = [1, 2, 19, 20, 21, 57, 78, 200, 1000]
    sizes = [1, 100, 4096, 4097, 10 ** 6, 44 * 10 ** 6, 10 ** 9, 10 ** 11]
    tab = [[int(lib.vog_opt_scratch_bytes(n, e)) for e in sizes] for n in counts]
    for i, row in enumerate(tab):
        for j, b in enumerate(row):
            assert b > 0
            assert j == 0 or b >= row[j - 1], (counts[i], sizes[j])
            assert i == 0 or b >= tab[i - 1][j], (counts[i], sizes[j])
    assert tab[-1][-1] > tab[0][0]


def test_opt_structs_match_the_header(tmp_path):
    """sizeof and every member offset of the three optimiser structs, as a C compiler lays them out, against the ctypes
    mirrors. The compiler is the system's, or the clang of the ROCm install the library itself is built with - so there is
    always one, and its absence is a failure (a skip would hide ABI drift)."""
    import os
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # (csrc/build.py's)
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang")
    found = [shutil.which(c) for c in ("cc", "gcc", "clang")] + [rocm_clang if os.access(rocm_clang, os.X_OK) else None]
    found = [c for c in found if c]
    assert found, f"no C compiler: none of cc, gcc, clang on PATH and no {rocm_clang}"
    gcc = found[0]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"vog_opt_tensor": L.OptTensor, "vog_opt_state": L.OptState, "vog_opt_args": L.OptArgs}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vog_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append(f'  printf("{cname} - %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            src.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    src += ['  return 0;', '}']
    cfile = tmp_path / "abi.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.run([gcc, "-I", os.path.join(root, "include"), str(cfile), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        cname, field, val = line.split()
        cls = pairs[cname]
        if field == "-":
            assert C.sizeof(cls) == int(val), (cname, C.sizeof(cls), val)
        else:
            assert getattr(cls, field).offset == int(val), (cname, field, val)
    assert C.sizeof(L.OptState) == 32
