"""The five *_scratch_bytes of the fp32 / amp training path (csrc/train_tx.hip, train_lang.hip) without a GPU: no kernel runs, a size is the
extent of the operator's layout walked without a base.

The rule the sizes follow (csrc/train_dev.h `Carve`): every carve advances by its bytes rounded up to the operator's padding
(vog_attn_f32: 4 floats, vog_lang_f32: 64 floats, the other three: 1 float), and the two operators that start at the next
256-byte boundary count the worst case for it, 255 bytes. So
    vog_attn_f32_scratch_bytes = 255 + a multiple of 16,    vog_lang_f32_scratch_bytes = 255 + a multiple of 256,
    the other three            = a multiple of 4."""
import importlib

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")
GRID = (1, 3, 8, 65)
# entry -> (base arguments, bytes in front of the padded carves, padding in bytes)
OPS = {"vog_mul_tail_bwd_scratch_bytes": ((3, 8, 3, 3), 0, 4), "vog_attn_f32_scratch_bytes": ((3, 3, 3, 8), 255, 16),
       "vog_linear_f32_scratch_bytes": ((3, 8), 0, 4), "vog_score_head_f32_bwd_scratch_bytes": ((3, 8, 3), 0, 4),
       "vog_lang_f32_scratch_bytes": ((3, 3, 3, 8, 3, 2, 8, 3), 255, 256)}          # (Bn, T, nsrl, E, R, layers, D, L)
LAYERS = 5                                                                           # position of `layers` in the language arguments


def _rows(fn):
    """-> [(dimension index, [arguments with that dimension walking the grid, the others at their base value])]"""
    base = OPS[fn][0]
    for i in range(len(base)):
        vals = (1, 2, 3, 4) if fn == "vog_lang_f32_scratch_bytes" and i == LAYERS else GRID
        yield i, [base[:i] + (v,) + base[i + 1:] for v in vals]


@pytest.mark.parametrize("fn", list(OPS))
@pytest.mark.parametrize("amp", [0, 1, 2])
def test_sizes_are_positive_monotone_and_follow_the_padding_rule(fn, amp):
    lib = L.load()
    f = getattr(lib, fn)
    _, lead, pad = OPS[fn]
    assert lib.vog_train_set_int(b"amp", amp) == 0
    try:
        for i, row in _rows(fn):
            sizes = [int(f(*a)) for a in row]
            for a, nb in zip(row, sizes):
                assert nb > 0, (fn, a)
                assert nb >= lead and (nb - lead) % pad == 0, (fn, a, nb)
            assert sizes == sorted(sizes), (fn, i, sizes)
        if fn == "vog_mul_tail_bwd_scratch_bytes":                                   # dhead = 0: a tail without the score head
            assert 0 < f(3, 8, 3, 0) <= f(3, 8, 3, 1)
    finally:
        lib.vog_train_set_int(b"amp", 0)


def test_language_size_follows_the_amp_switch_and_returns():
    lib = L.load()
    f = lib.vog_lang_f32_scratch_bytes
    for _, row in _rows("vog_lang_f32_scratch_bytes"):
        for a in row:
            off = int(f(*a))
            for amp in (1, 2):
                assert lib.vog_train_set_int(b"amp", amp) == 0
                try:
                    on = int(f(*a))
                finally:
                    lib.vog_train_set_int(b"amp", 0)
                assert on > off, (a, amp, on, off)
                assert int(f(*a)) == off, (a, amp)


def test_only_the_language_size_depends_on_amp():
    lib = L.load()
    for fn, (base, _, _) in OPS.items():
        if fn == "vog_lang_f32_scratch_bytes":
            continue
        off = int(getattr(lib, fn)(*base))
        assert lib.vog_train_set_int(b"amp", 1) == 0
        try:
            assert int(getattr(lib, fn)(*base)) == off, fn
        finally:
            lib.vog_train_set_int(b"amp", 0)
