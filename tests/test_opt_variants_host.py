"""Host side of the optimiser variants (no GPU): the C ABI of vog_opt_step_ex_f32 / vog_opt_accum_f32 (include/vog_hip.h) and
their argument checks, which run before any launch; the `cfg.hip` optimiser keys, their CLI spelling and refusals; the trainer
arguments that are checked before any device work; and the learning-rate glue (`trn_utils.LRSchedule`) against torch's own
schedulers on a real torch.optim.Adam."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest
import torch

L = importlib.import_module("vognet-pytorch_amd.lib")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
trn = importlib.import_module("vognet-pytorch_amd.train")

FAKE = 0x10000          # never dereferenced: a faulty call returns before it touches the device
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- ABI
def test_new_structs_match_the_header_and_the_entries_are_built(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang")
    found = [shutil.which(c) for c in ("gcc", "cc", "clang")] + [rocm_clang if os.access(rocm_clang, os.X_OK) else None]
    found = [c for c in found if c]
    assert found, f"no C compiler: none of gcc, cc, clang on PATH and no {rocm_clang}"
    pairs = {"vog_opt_ex_args": L.OptExArgs, "vog_opt_accum_tensor": L.OptAccumTensor}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vog_hip.h"', 'int main(void) {',
           '  printf("flags - %u\\n", VOG_OPT_DECOUPLED | VOG_OPT_AMSGRAD << 8 | VOG_OPT_MAXIMIZE << 16);']
    for cname, cls in pairs.items():
        src.append(f'  printf("{cname} - %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            src.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    src += ['  return 0;', '}']
    cfile = tmp_path / "abi.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.run([found[0], "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        cname, field, val = line.split()
        if cname == "flags":
            assert int(val) == L.OPT_DECOUPLED | L.OPT_AMSGRAD << 8 | L.OPT_MAXIMIZE << 16
            continue
        cls = pairs[cname]
        if field == "-":
            assert C.sizeof(cls) == int(val), (cname, C.sizeof(cls), val)
        else:
            assert getattr(cls, field).offset == int(val), (cname, field, val)
        seen += 1
    assert seen == 2 + 4 + 3
    assert L.OptExArgs.groups.offset == 0 and L.OptExArgs.groups.size == C.sizeof(L.OptGroupsArgs)
    lib = L.load()
    for name in ("vog_opt_step_ex_f32", "vog_opt_accum_f32"):
        assert name in L.SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "vog_hip.h")).read()
    assert "int vog_opt_step_ex_f32(const vog_opt_ex_args* a, void* stream);" in header
    assert "int vog_opt_accum_f32(const vog_opt_accum_tensor* tensors, int n_tensors, void* stream);" in header
    assert "NOT AdamW" not in header and "VOG_OPT_DECOUPLED" in header


def _exargs(groups=((0, 2, 1e-3, 0.0), (4, 2, 1e-3, 0.01)), n_tensors=6, mode_b=False, flags=0, grad_scale=1.0, vmax=True):
    arr = (L.OptTensor * n_tensors)()
    for i in range(n_tensors):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, 100
    ex = L.OptExArgs()
    a = ex.groups.base
    a.tensors, a.n_tensors = arr, n_tensors
    a.lr, a.beta1, a.beta2, a.eps, a.step = 1e-3, 0.9, 0.99, 1e-8, 1
    if mode_b:
        a.state, a.scratch = FAKE + 0x4000, FAKE + 0x5000
        a.scratch_bytes = int(L.load().vog_opt_scratch_bytes(n_tensors, 100 * n_tensors))
        a.growth_factor, a.backoff_factor, a.growth_interval = 2.0, 0.5, 2000
    garr = (L.OptGroup * max(len(groups), 1))()
    for i, (first, count, lr, wd) in enumerate(groups):
        garr[i].first, garr[i].count, garr[i].lr, garr[i].weight_decay = first, count, lr, wd
    ex.groups.groups, ex.groups.n_groups = garr, len(groups)
    vm = (C.c_void_p * n_tensors)()
    for i in range(n_tensors):
        vm[i] = FAKE + 0x6000
    if vmax:
        ex.vmax = vm
    ex.flags, ex.grad_scale = flags, grad_scale
    return ex, (arr, garr, vm)


def _vmax_null(ex, keep):
    keep[2][5] = None                       # tensor 5 is in the second group


def _vmax_misaligned(ex, keep):
    keep[2][0] = FAKE + 0x6002


def _tensor_misaligned(ex, keep):
    keep[0][1].m = FAKE + 0x2001


def _set(**kw):
    def f(ex, keep):
        for k, v in kw.items():
            setattr(ex, k, v)
    return f


def _no_vmax_table(ex, keep):
    ex.vmax = C.POINTER(C.c_void_p)()


EX_FAULTS = {
    "vmax NULL for a grouped tensor": (L.OPT_AMSGRAD, _vmax_null, b"vmax[5]"),
    "vmax misaligned": (L.OPT_AMSGRAD, _vmax_misaligned, b"vmax[0]"),
    "no vmax table": (L.OPT_AMSGRAD | L.OPT_DECOUPLED, _no_vmax_table, b"vmax"),
    "tensor pointer misaligned": (L.OPT_DECOUPLED, _tensor_misaligned, b"& 3"),
    "grad_scale zero": (0, _set(grad_scale=0.0), b"grad_scale"),
    "grad_scale negative": (L.OPT_MAXIMIZE, _set(grad_scale=-0.5), b"grad_scale"),
    "grad_scale nan": (0, _set(grad_scale=float("nan")), b"grad_scale"),
    "grad_scale inf": (0, _set(grad_scale=float("inf")), b"grad_scale"),
    "unknown flag bit": (0, _set(flags=8), b"flag"),
    "unknown high flag bit": (L.OPT_AMSGRAD, _set(flags=L.OPT_AMSGRAD | 1 << 31), b"flag"),
}


@pytest.mark.parametrize("mode_b", [False, True])
@pytest.mark.parametrize("fault", sorted(EX_FAULTS))
def test_ex_argument_errors_come_back_before_any_device_call(fault, mode_b):
    """The pointers are fakes: a call that got as far as a launch (or a device read) would crash, not return."""
    lib = L.load()
    flags, spoil, word = EX_FAULTS[fault]
    ex, keep = _exargs(mode_b=mode_b, flags=flags)
    spoil(ex, keep)
    assert lib.vog_opt_step_ex_f32(C.byref(ex), None) != 0
    assert word in lib.vog_last_error(), (fault, lib.vog_last_error())


def test_ex_entry_keeps_the_grouped_steps_checks():
    lib = L.load()
    assert lib.vog_opt_step_ex_f32(None, None) != 0
    for groups, word in (([(0, 3, 1e-3, 0.0), (2, 2, 1e-3, 0.0)], b"ascending"), ([(0, 2, 1e-3, 0.0), (4, 3, 1e-3, 0.0)], b"the table has 6"),
                         ([(0, 2, -1e-3, 0.0)], b"lr"), ([], b"n_groups")):
        ex, keep = _exargs(groups=groups, flags=L.OPT_AMSGRAD)
        assert lib.vog_opt_step_ex_f32(C.byref(ex), None) != 0 and word in lib.vog_last_error(), (groups, lib.vog_last_error())
    ex, keep = _exargs(flags=L.OPT_DECOUPLED)
    ex.groups.base.step = 0
    assert lib.vog_opt_step_ex_f32(C.byref(ex), None) != 0 and b"step" in lib.vog_last_error()
    ex, keep = _exargs(groups=[(0, 6, 1e-3, 0.0)], flags=L.OPT_AMSGRAD, mode_b=True)
    ex.groups.base.scratch_bytes -= 1
    assert lib.vog_opt_step_ex_f32(C.byref(ex), None) != 0 and b"scratch" in lib.vog_last_error()
    # the messages name the entry that was called
    ex, keep = _exargs(groups=[(0, 0, 1e-3, 0.0)])
    assert lib.vog_opt_step_ex_f32(C.byref(ex), None) != 0 and b"vog_opt_step_ex_f32" in lib.vog_last_error()


def _accum(n=3):
    arr = (L.OptAccumTensor * n)()
    for i in range(n):
        arr[i].acc, arr[i].g, arr[i].n = FAKE, FAKE + 0x1000, 100
    return arr


@pytest.mark.parametrize("fault, word", [("acc", b"NULL"), ("g", b"NULL"), ("n0", b"n = 0"), ("nneg", b"n = -1"),
                                         ("misaligned acc", b"aligned"), ("misaligned g", b"aligned")])
def test_accum_argument_errors_come_back_before_any_device_call(fault, word):
    lib = L.load()
    arr = _accum(40)                        # (more than one launch's table: the fault sits in the second)
    t = arr[35]
    if fault == "acc":
        t.acc = None
    elif fault == "g":
        t.g = None
    elif fault == "n0":
        t.n = 0
    elif fault == "nneg":
        t.n = -1
    elif fault == "misaligned acc":
        t.acc = FAKE + 2
    else:
        t.g = FAKE + 0x1001
    assert lib.vog_opt_accum_f32(arr, 40, None) != 0
    err = lib.vog_last_error()
    assert word in err and b"tensor 35" in err, err


def test_accum_entry_refuses_an_empty_table():
    lib = L.load()
    assert lib.vog_opt_accum_f32(None, 3, None) != 0
    assert lib.vog_opt_accum_f32(_accum(3), 0, None) != 0
    assert lib.vog_opt_accum_f32(_accum(3), -1, None) != 0


# ---------------------------------------------------------------- config, CLI
def test_optimizer_config_keys_defaults_cli_and_refusals():
    cfg = ec.get_default_cfg()
    assert (cfg.hip.train_optimizer, cfg.hip.train_amsgrad, cfg.hip.train_accum_steps) == ("adam", False, 1)
    assert (cfg.hip.train_plateau_factor, cfg.hip.train_plateau_patience) == (0.1, 10)
    assert tu.train_optimizer(cfg) == {"optimizer": "adam", "amsgrad": False, "accum_steps": 1, "plateau_factor": 0.1,
                                       "plateau_patience": 10}
    uid, kw = main_mod.parse_argv(["run1", "--hip.train_optimizer=adamw", "--hip.train_amsgrad", "--hip.train_accum_steps=4",
                                   "--hip.train_plateau_factor=0.5", "--hip.train_plateau_patience", "0",
                                   "--train.use_reduce_lr_plateau=True"])
    ec.update_from_dict(cfg, kw)
    ec.post_proc_config(cfg)
    assert tu.train_optimizer(cfg) == {"optimizer": "adamw", "amsgrad": True, "accum_steps": 4, "plateau_factor": 0.5,
                                       "plateau_patience": 0}
    assert cfg.train.use_reduce_lr_plateau is True
    with pytest.raises(AssertionError):                         # the type of the default is enforced by update_from_dict
        ec.update_from_dict(cfg, {"hip.train_accum_steps": "2.5"})
    for key, bad in (("train_optimizer", "sgd"), ("train_optimizer", ""), ("train_accum_steps", 0), ("train_accum_steps", -2),
                     ("train_accum_steps", True), ("train_plateau_factor", 0.0), ("train_plateau_factor", 1.0),
                     ("train_plateau_factor", -0.5), ("train_plateau_factor", 1.5), ("train_plateau_patience", -1),
                     ("train_amsgrad", "yes")):
        c = ec.get_default_cfg()
        c.hip[key] = bad
        for check in (ec.check_hip_options, ec.post_proc_config, tu.train_optimizer):
            with pytest.raises(ValueError, match=key):
                check(c)
    c = ec.get_default_cfg()
    del c["hip"]                                                # a reference config has no hip section: the defaults
    assert tu.train_optimizer(c)["optimizer"] == "adam" and tu.train_optimizer(c)["accum_steps"] == 1
    for key in ("train_optimizer", "train_amsgrad", "train_accum_steps", "train_plateau_factor", "train_plateau_patience"):
        assert f"--hip.{key}" in main_mod.__doc__, key


# ---------------------------------------------------------------- trainer arguments
@pytest.mark.parametrize("kw, word", [
    (dict(optimizer="sgd"), "optimizer"), (dict(optimizer=None), "optimizer"), (dict(optimizer="AdamW"), "optimizer"),
    (dict(accum_steps=0), "accum_steps"), (dict(accum_steps=-1), "accum_steps"), (dict(accum_steps=1.5), "accum_steps"),
    (dict(accum_steps=True), "accum_steps"), (dict(amsgrad=1), "amsgrad"), (dict(maximize="no"), "maximize"),
])
def test_trainer_arguments_are_checked_before_any_device_work(kw, word):
    """cfg, comm and the loss are None: a constructor that got past its argument checks would fail on them (or on the
    missing GPU), not with a ValueError that names the argument."""
    with pytest.raises(ValueError, match=word):
        trn.FP32Trainer(None, None, {}, None, lr=1e-4, **kw)
    with pytest.raises(ValueError, match=word):
        trn.parse_optimizer(**{"optimizer": "adam", **kw})


def test_trainer_argument_defaults_and_group_refusals_stay():
    assert trn.parse_optimizer("adam") == ("adam", False, False, 1)
    assert trn.parse_optimizer("adamw", True, True, 3) == ("adamw", True, True, 3)
    for flag in ("amsgrad", "maximize"):                        # trainer-wide, still no per-group setting
        with pytest.raises(ValueError, match=flag):
            trn.resolve_param_groups(["a.w", "b.w"], [{"params": ["a."], flag: True}])


# ---------------------------------------------------------------- learning-rate sequences
METRICS = [0.3, 0.31, 0.32, 0.33, 0.2, 0.25, 0.26]


def _torch_adam(lrs):
    return torch.optim.Adam([{"params": [torch.zeros(2, requires_grad=True)], "lr": lr} for lr in lrs], lr=1.0)


def test_plateau_rates_are_torchs_own_floats_and_survive_a_state_dict_round_trip():
    lrs0 = [1e-4, 3e-5]
    opt = _torch_adam(lrs0)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=1)
    glue = tu.LRSchedule(lrs0, plateau=True, factor=0.5, patience=1)
    assert glue.lrs() == lrs0
    want, got = [], []
    for i, m in enumerate(METRICS):
        ref.step(m)
        want.append([g["lr"] for g in opt.param_groups])
        got.append(glue.step(m))
        if i == 4:                                              # mid-sequence: what a checkpoint holds
            saved, saved_lrs = glue.state_dict(), glue.lrs()
    assert got == want, (got, want)                             # equal as Python floats
    assert want[-1] != lrs0 and len({tuple(x) for x in want}) >= 3          # the script makes the rate fall more than once
    # a fresh schedule over the restored rates, with the saved state, continues the same sequence
    resumed = tu.LRSchedule(saved_lrs, plateau=True, factor=0.5, patience=1)
    resumed.load_state_dict(saved)
    assert [resumed.step(m) for m in METRICS[5:]] == want[5:]
    # without the state the continuation differs (the state is what carries best / num_bad_epochs)
    fresh = tu.LRSchedule(saved_lrs, plateau=True, factor=0.5, patience=1)
    assert [fresh.step(m) for m in METRICS[5:]] != want[5:]


def test_default_schedule_is_the_references_constant_lambda():
    lrs0 = [1e-4, 3e-5]
    opt = _torch_adam(lrs0)
    ref = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 1)
    glue = tu.LRSchedule(lrs0)
    for m in METRICS:
        ref.step()
        assert glue.step(m) == [g["lr"] for g in opt.param_groups] == lrs0
    again = tu.LRSchedule(lrs0)
    again.load_state_dict(glue.state_dict())
    assert again.step(None) == lrs0
