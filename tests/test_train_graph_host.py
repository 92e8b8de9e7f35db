"""The captured training step without a GPU: the option `cfg.hip.train_graph` on its surfaces, the rules by which a capture is
refused, the host-built bias-correction table of the device-counted optimiser (`vog_opt_bias_table`), the device-counted dropout
seed against `FP32Trainer._step_seed` restated, and the ctypes mirrors of the two new structs against the C header."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
EC = importlib.import_module("vognet-pytorch_amd.extended_config")
TR = importlib.import_module("vognet-pytorch_amd.train")
TU = importlib.import_module("vognet-pytorch_amd.trn_utils")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 0x7FFFFFFFFFFFFFFF


def test_option_is_parsed_on_every_surface():
    assert EC.parse_train_graph({}) is False and EC.parse_train_graph({"train_graph": True}) is True
    for bad in ("", "True", 1, 0, None):
        with pytest.raises(ValueError, match="train_graph"):
            EC.parse_train_graph({"train_graph": bad})

    class Cfg(dict):
        pass

    EC.check_hip_options(Cfg(hip={"train_graph": True}))
    with pytest.raises(ValueError, match="train_graph"):
        EC.check_hip_options(Cfg(hip={"train_graph": "yes"}))
    assert TU.train_graph(Cfg(hip={"train_graph": True})) is True and TU.train_graph(Cfg()) is False
    # the command line of main_dist: --hip.train_graph=True arrives as text and lands as a bool; off by default
    cfg = EC.get_default_cfg()
    assert cfg.hip.train_graph is False
    EC.update_from_dict(cfg, {"hip.train_graph": "True"})
    assert cfg.hip.train_graph is True
    with pytest.raises(AssertionError):
        EC.update_from_dict(cfg, {"hip.train_graph": "maybe"})
    doc = importlib.import_module("vognet-pytorch_amd.main_dist").__doc__
    assert "--hip.train_graph=True" in doc


@pytest.mark.parametrize("accum,world,path,word", [(1, 1, "trainer", None), (2, 1, "trainer", "accum_steps"), (1, 2, "trainer", "ranks"),
                                                   (1, 1, "autograd", "autograd"), (4, 8, "trainer", "accum_steps"),
                                                   (1, 4, "autograd", "autograd")])
def test_refusal_rules(accum, world, path, word):
    why = TR.capture_refusal(accum, world, path)
    if word is None:
        assert why is None
    else:
        assert why is not None and word in why and "eager" in why


def _table(b1, b2, cap):
    lib = L.load()
    out = (C.c_float * (2 * cap + 2))(*([-7.0] * (2 * cap + 2)))
    n = C.c_int(-1)
    rc = lib.vog_opt_bias_table(b1, b2, out, cap, C.byref(n))
    return rc, n.value, np.frombuffer(out, dtype=np.float32).copy()


def test_bias_table_ends_where_both_corrections_are_one():
    rc, n, t = _table(0.9, 0.99, 4096)
    assert rc == 0
    # numpy's float32 power gives 1725 here; libm's may differ from it in a last bit
    assert abs(n - 1725) <= 2, n
    pairs = t[:2 * n].reshape(n, 2)
    assert np.all(np.diff(pairs[:, 0]) >= 0) and np.all(np.diff(pairs[:, 1]) >= 0)
    assert tuple(pairs[-1]) == (1.0, 1.0) and tuple(pairs[-2]) != (1.0, 1.0)
    assert not np.any((pairs[:-1, 0] == 1.0) & (pairs[:-1, 1] == 1.0))
    assert np.all(t[2 * n:] == -7.0)                                    # nothing behind the last entry
    # the entries are mode A's own expressions (float32 throughout; one last bit of libm's power against numpy's)
    s = np.arange(1, 9, dtype=np.float32)
    b1, b2 = np.float32(0.9), np.float32(0.99)
    np.testing.assert_allclose(pairs[:8, 0], np.float32(1) - np.power(b1, s), rtol=3e-7)
    np.testing.assert_allclose(pairs[:8, 1], np.sqrt(np.float32(1) - np.power(b2, s)), rtol=3e-7)
    assert pairs[0, 0] == np.float32(1) - b1


def test_bias_table_respects_its_capacity():
    rc, n, t = _table(0.9, 0.99, 100)
    assert rc == -2 and abs(n - 1725) <= 2
    assert b"entries" in L.load().vog_last_error()
    assert np.all(t[:200] != -7.0) and np.all(t[200:] == -7.0)          # the first cap entries, and not one float more
    full = _table(0.9, 0.99, 4096)[2]
    assert np.array_equal(t[:200], full[:200])
    lib, n = L.load(), C.c_int(0)
    assert lib.vog_opt_bias_table(0.9, 0.99, None, 0, C.byref(n)) == -2 and abs(n.value - 1725) <= 2      # a pure count
    assert lib.vog_opt_bias_table(0.9, 1.0, None, 0, C.byref(n)) == -1                                       # beta2 = 1 never ends
    assert lib.vog_opt_bias_table(0.9, 0.99, None, 0, None) == -1


def test_bias_table_refuses_more_than_2_pow_20_entries():
    lib, n = L.load(), C.c_int(0)
    assert lib.vog_opt_bias_table(0.9, 0.99999, None, 0, C.byref(n)) == -2
    assert n.value > TR.BIAS_TABLE_MAX and b"2^20" in lib.vog_last_error()


def _step_seed(dropout_seed, num_it):
    """FP32Trainer._step_seed, restated."""
    return (dropout_seed * 1000003 + num_it + 1) & MASK


@pytest.mark.parametrize("seed", [0, 1, 1234, 0x7FFFFFFF, 2 ** 44 + 3, 2 ** 45, 2 ** 63 - 1, 2 ** 64 // 1000003 + 1, 2 ** 70 + 12345])
def test_device_seed_rule_is_the_hosts_step_seed(seed):
    """What the kernels compute with a tick pointer - (base + tick) mod 2^64, masked to 63 bits, base = seed * 1000003 + 1 mod
    2^64 - against the host's arbitrary-precision expression, with seeds whose product passes 2^64 (and 2^63) among them."""
    base = TR.step_seed_base(seed)
    assert 0 <= base < 2 ** 64 and base == (seed * 1000003 + 1) % 2 ** 64
    for tick in (0, 1, 2, 999, 2 ** 31, 2 ** 40 + 7, 2 ** 63 - base % 2 ** 63, 2 ** 64 - base):
        dev = ((base + tick) % 2 ** 64) & MASK
        assert dev == _step_seed(seed, tick), (seed, tick)


def test_ctypes_structs_match_the_c_header(tmp_path):
    structs = {"vog_train_step": L.TrainStep, "vog_opt_dev_args": L.OptDevArgs}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {n} %zu\\n", offsetof({cname}, {n}));' for n, _ in cls._fields_]
    prog = tmp_path / "lay.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vog_hip.h"\nint main(void) {\n' + "\n".join(lines)
                    + "\n  return 0;\n}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    rows = [ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = {(a, b): int(c) for a, b, c in rows}
    for cname, cls in structs.items():
        assert got[(cname, "sizeof")] == C.sizeof(cls), cname
        for n, _ in cls._fields_:
            assert got[(cname, n)] == getattr(cls, n).offset, (cname, n)
    assert C.sizeof(L.TrainStep) == 16 and L.TrainStep.len_clamped.offset == 12


def test_pointer_switch_and_pin_are_refused_and_reported_without_a_device():
    lib = L.load()
    assert lib.vog_train_set_ptr(b"drop_tick", None) == 0
    assert lib.vog_train_set_ptr(b"no_such_pointer", None) == -1 and b"no_such_pointer" in lib.vog_last_error()
    assert lib.vog_train_set_ptr(b"drop_tick", 12) == -1 and b"aligned" in lib.vog_last_error()
    assert lib.vog_train_set_ptr(None, None) == -1
    p, n, pin = C.c_void_p(1), C.c_size_t(1), C.c_int(1)
    fake = 0x1000                                                       # a stream handle nothing was ever launched on
    assert lib.vog_train_scratch_info(fake, C.byref(p), C.byref(n), C.byref(pin)) == 0
    assert (p.value, n.value, pin.value) == (None, 0, 0)
    assert lib.vog_train_pin_scratch(fake, 1) == 0
    assert lib.vog_train_scratch_info(fake, C.byref(p), C.byref(n), C.byref(pin)) == 0 and (p.value, n.value, pin.value) == (None, 0, 1)
    assert lib.vog_train_pin_scratch(fake, 0) == 0
    assert lib.vog_train_scratch_info(fake, None, None, C.byref(pin)) == 0 and pin.value == 0
    # the tick's argument errors come back before any launch
    assert lib.vog_train_tick(None, None, 0, 0, None, None, 0, 0, L.TICK_BEGIN, 0, None, 0, None) == -1
