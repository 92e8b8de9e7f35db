"""Host side of weight averaging (no GPU): the C ABI of vog_opt_average_f32 (include/vog_hip.h) and its argument checks, which
run before any launch; the `cfg.hip.train_avg*` keys, their CLI spelling and refusals; the trainer arguments that are checked
before any device work; and that the defaults switch everything off."""
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
AVG_KEYS = ("train_avg", "train_avg_decay", "train_avg_warmup", "train_avg_start", "train_avg_every", "train_avg_eval")


# ---------------------------------------------------------------- ABI
def test_averaging_structs_match_the_header_and_the_entry_is_built(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang")
    found = [shutil.which(c) for c in ("gcc", "cc", "clang")] + [rocm_clang if os.access(rocm_clang, os.X_OK) else None]
    found = [c for c in found if c]
    assert found, f"no C compiler: none of gcc, cc, clang on PATH and no {rocm_clang}"
    pairs = {"vog_opt_avg_tensor": L.OptAvgTensor, "vog_opt_avg_state": L.OptAvgState, "vog_opt_avg_args": L.OptAvgArgs}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vog_hip.h"', 'int main(void) {',
           '  printf("modes - %d\\n", VOG_AVG_EMA | VOG_AVG_SWA << 8);']
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
        if cname == "modes":
            assert int(val) == L.AVG_EMA | L.AVG_SWA << 8
            continue
        cls = pairs[cname]
        if field == "-":
            assert C.sizeof(cls) == int(val), (cname, C.sizeof(cls), val)
        else:
            assert getattr(cls, field).offset == int(val), (cname, field, val)
        seen += 1
    assert seen == 3 + 3 + 4 + 10
    assert C.sizeof(L.OptAvgState) == 16
    lib = L.load()
    assert "vog_opt_average_f32" in L.SYMBOLS and lib.vog_opt_average_f32 is not None
    header = open(os.path.join(ROOT, "include", "vog_hip.h")).read()
    assert "int vog_opt_average_f32(const vog_opt_avg_args* a, void* stream);" in header


def _args(n=40, mode=None, mode_b=False):
    arr = (L.OptAvgTensor * n)()
    for i in range(n):
        arr[i].avg, arr[i].p, arr[i].n = FAKE, FAKE + 0x1000, 100
    a = L.OptAvgArgs()
    a.tensors, a.n_tensors = arr, n
    a.mode, a.decay, a.warmup, a.start, a.every = (L.AVG_EMA if mode is None else mode), 0.999, 0, 1, 1
    a.state = FAKE + 0x2000
    if mode_b:
        a.opt_state = FAKE + 0x3000
    else:
        a.step = 1
    return a, arr


def _tensor(**kw):
    def f(a, arr):
        for k, v in kw.items():
            setattr(arr[35], k, v)           # (more than one launch's table: the fault sits in the second)
    return f


def _set(**kw):
    def f(a, arr):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


AVG_FAULTS = {
    "avg NULL": (_tensor(avg=None), b"tensor 35"),
    "p NULL": (_tensor(p=None), b"tensor 35"),
    "avg misaligned": (_tensor(avg=FAKE + 2), b"tensor 35"),
    "p misaligned": (_tensor(p=FAKE + 0x1001), b"tensor 35"),
    "n zero": (_tensor(n=0), b"tensor 35"),
    "n negative": (_tensor(n=-1), b"tensor 35"),
    "mode unknown": (_set(mode=3), b"mode"),
    "mode zero": (_set(mode=0), b"mode"),
    "decay negative": (_set(decay=-0.1), b"decay"),
    "decay above one": (_set(decay=1.0000001), b"decay"),
    "decay nan": (_set(decay=float("nan")), b"decay"),
    "decay inf": (_set(decay=float("inf")), b"decay"),
    "start zero": (_set(start=0), b"start"),
    "every zero": (_set(every=0), b"every"),
    "every negative": (_set(every=-3), b"every"),
    "state NULL": (_set(state=None), b"state"),
}


@pytest.mark.parametrize("mode_b", [False, True])
@pytest.mark.parametrize("fault", sorted(AVG_FAULTS))
def test_average_argument_errors_come_back_before_any_device_call(fault, mode_b):
    """The pointers are fakes: a call that got as far as a launch (or a device read) would crash, not return."""
    lib = L.load()
    spoil, word = AVG_FAULTS[fault]
    a, arr = _args(mode_b=mode_b)
    spoil(a, arr)
    assert lib.vog_opt_average_f32(C.byref(a), None) != 0
    err = lib.vog_last_error()
    assert word in err and (b"vog_opt_average_f32" in err or b"optim.hip" in err), (fault, err)


def test_average_entry_refuses_mode_a_without_a_step_and_an_empty_table():
    lib = L.load()
    assert lib.vog_opt_average_f32(None, None) != 0
    for step in (0, -1):
        a, arr = _args()
        a.step = step
        assert lib.vog_opt_average_f32(C.byref(a), None) != 0 and b"step" in lib.vog_last_error()
    a, arr = _args()
    a.n_tensors = 0
    assert lib.vog_opt_average_f32(C.byref(a), None) != 0
    a, arr = _args()
    a.tensors = C.POINTER(L.OptAvgTensor)()
    assert lib.vog_opt_average_f32(C.byref(a), None) != 0
    # SWA does not read the decay: whatever it holds is no error of an SWA call - a tensor fault still is
    a, arr = _args(mode=L.AVG_SWA)
    a.decay = float("nan")
    arr[0].n = 0
    assert lib.vog_opt_average_f32(C.byref(a), None) != 0 and b"tensor 0" in lib.vog_last_error()


# ---------------------------------------------------------------- config, CLI
def test_averaging_config_keys_defaults_cli_and_refusals():
    cfg = ec.get_default_cfg()
    assert [cfg.hip[k] for k in AVG_KEYS] == ["", 0.999, False, 1, 1, False]
    off = {"avg": None, "decay": 0.999, "warmup": False, "start": 1, "every": 1, "eval": False}
    assert tu.train_avg(cfg) == off == ec.parse_train_avg(cfg.hip)
    uid, kw = main_mod.parse_argv(["run1", "--hip.train_avg=ema", "--hip.train_avg_decay=0.99", "--hip.train_avg_warmup",
                                   "--hip.train_avg_start", "5", "--hip.train_avg_every=4", "--hip.train_avg_eval=True"])
    ec.update_from_dict(cfg, kw)
    ec.post_proc_config(cfg)
    assert tu.train_avg(cfg) == {"avg": "ema", "decay": 0.99, "warmup": True, "start": 5, "every": 4, "eval": True}
    c = ec.get_default_cfg()
    ec.update_from_dict(c, {"hip.train_avg": "swa", "hip.train_avg_decay": "1"})         # (an int where the default is a float)
    assert tu.train_avg(c)["avg"] == "swa" and tu.train_avg(c)["decay"] == 1.0
    with pytest.raises(AssertionError):                         # the type of the default is enforced by update_from_dict
        ec.update_from_dict(cfg, {"hip.train_avg_every": "2.5"})
    for key, bad in (("train_avg", "mean"), ("train_avg", "EMA"), ("train_avg_decay", -0.1), ("train_avg_decay", 1.5),
                     ("train_avg_decay", float("nan")), ("train_avg_decay", True), ("train_avg_warmup", "yes"),
                     ("train_avg_start", 0), ("train_avg_start", True), ("train_avg_every", 0), ("train_avg_every", -2),
                     ("train_avg_every", 1.5), ("train_avg_eval", "yes")):
        c = ec.get_default_cfg()
        c.hip.train_avg = "ema"
        c.hip[key] = bad
        for check in (ec.check_hip_options, ec.post_proc_config, tu.train_avg):
            with pytest.raises(ValueError, match=key):
                check(c)
    c = ec.get_default_cfg()
    c.hip.train_avg_eval = True                                 # nothing to evaluate without an average
    for check in (ec.check_hip_options, ec.post_proc_config, tu.train_avg):
        with pytest.raises(ValueError, match="train_avg_eval"):
            check(c)
    c = ec.get_default_cfg()
    del c["hip"]                                                # a reference config has no hip section: the defaults
    assert tu.train_avg(c) == off
    for key in AVG_KEYS:
        assert key in main_mod.__doc__, key
    assert "--hip.train_avg=ema" in main_mod.__doc__ and "--hip.train_avg_eval=True" in main_mod.__doc__


def test_a_checkpoint_without_the_averaging_key_is_refused_for_averaged_evaluation():
    sd = {"module.a.w": torch.ones(3), "b.w": torch.zeros(2)}
    with pytest.raises(ValueError, match="averaging_state_dict"):
        tu.averaged_weights_from_checkpoint({"model_state_dict": sd})
    asd = {"mode": "ema", "n_averaged": 2, "averaged": {"a.w": torch.full((3,), 5.0)}}
    got = tu.averaged_weights_from_checkpoint({"model_state_dict": sd, "averaging_state_dict": asd})
    assert set(got) == {"a.w", "b.w"} and torch.equal(got["a.w"], torch.full((3,), 5.0)) and torch.equal(got["b.w"], torch.zeros(2))
    # saved before the first averaging update: every parameter is its own average
    asd0 = {"mode": "ema", "n_averaged": 0, "averaged": {"a.w": torch.zeros(3)}}
    got = tu.averaged_weights_from_checkpoint({"model_state_dict": sd, "averaging_state_dict": asd0})
    assert torch.equal(got["a.w"], torch.ones(3))


# ---------------------------------------------------------------- trainer arguments
@pytest.mark.parametrize("kw, word", [
    (dict(avg="mean"), "avg"), (dict(avg="EMA"), "avg"), (dict(avg=True), "avg"), (dict(avg=""), "avg"),
    (dict(avg="ema", avg_decay=-0.1), "avg_decay"), (dict(avg="ema", avg_decay=1.01), "avg_decay"),
    (dict(avg="ema", avg_decay=float("nan")), "avg_decay"), (dict(avg="ema", avg_decay="0.9"), "avg_decay"),
    (dict(avg="ema", avg_warmup=1), "avg_warmup"), (dict(avg="swa", avg_start=0), "avg_start"),
    (dict(avg="swa", avg_start=1.0), "avg_start"), (dict(avg="swa", avg_every=0), "avg_every"),
    (dict(avg="swa", avg_every=True), "avg_every"),
])
def test_trainer_averaging_arguments_are_checked_before_any_device_work(kw, word):
    """cfg, comm and the loss are None: a constructor that got past its argument checks would fail on them (or on the
    missing GPU), not with a ValueError that names the argument."""
    with pytest.raises(ValueError, match=word):
        trn.FP32Trainer(None, None, {}, None, lr=1e-4, **kw)
    with pytest.raises(ValueError, match=word):
        trn.parse_averaging(**kw)


def test_the_defaults_switch_averaging_off(monkeypatch):
    assert trn.parse_averaging() == (None, 0.999, False, 1, 1)
    assert trn.parse_averaging("swa", 0.5, True, 3, 2) == ("swa", 0.5, True, 3, 2)
    assert trn.AVG_MODES == {"ema": L.AVG_EMA, "swa": L.AVG_SWA} and tuple(trn.AVG_MODES) == ec.TRAIN_AVG_MODES
    # a default trainer's update makes the optimiser call and nothing else: no averaging call, no averages, no state block
    calls = []
    t = object.__new__(trn.FP32Trainer)
    t.avg_mode, t.avg, t._avg_state = trn.parse_averaging()[0], {}, None
    monkeypatch.setattr(trn.FP32Trainer, "_adam_call", lambda self, grads, grad_scale=1.0: calls.append("adam") or ["k"])
    monkeypatch.setattr(trn.FP32Trainer, "_average", lambda self, keys: calls.append("average"))
    t._optimizer_step({"k": None})
    assert calls == ["adam"] and t.avg == {} and t._avg_state is None
    assert t.averaging_state_dict() is None and t.avg_state() == {"n_averaged": 0, "updated": 0, "w": 0.0}
    with pytest.raises(ValueError, match="avg"):
        t.averaged_state_dict()
    t.avg_mode = "ema"
    t._optimizer_step({"k": None})
    assert calls == ["adam", "adam", "average"]
    # the default cfg hands the trainer no averaging argument
    assert tu.train_avg(ec.get_default_cfg())["avg"] is None and tu.train_avg(ec.get_default_cfg())["eval"] is False
