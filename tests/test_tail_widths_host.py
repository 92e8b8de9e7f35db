"""Without a GPU: the shapes the fused encoder-layer tail admits (csrc/txtail.hip: tx_tail_supported, exported as
vog_tx_tail_supported). d = 256 and d = 384 (vsrl.*_encode_size = 128) joined d = 512 / 768; each width states its own rule for
kwo = heads x padded head width."""
import importlib

import pytest

L = importlib.import_module("vognet-pytorch_amd.lib")

KWO = {256: (256, 320, 384), 384: (384, 512, 640)}


@pytest.mark.parametrize("d,dh,kwo,want", [
    (256, 128, 384, 1), (384, 192, 384, 1),
    (512, 256, 576, 1), (768, 384, 768, 1), (768, 384, 576, 1), (768, 384, 640, 0), (512, 255, 576, 0), (320, 160, 320, 0),
    (1024, 512, 768, 0)])
def test_probe_table(d, dh, kwo, want):
    """The first two rows are new; the others are what the probe answered before them and must keep answering. (768, 384, 576) is
    1: 576 = 3 x 192, 36 k-steps walked three at a time; the 768-wide refusal next to it is 640.)"""
    assert L.load().vog_tx_tail_supported(d, dh, kwo) == want


@pytest.mark.parametrize("d", sorted(KWO))
def test_kwo_rule_of_the_narrow_widths(d):
    """every kwo of the stated rule is taken; every other multiple of 16 up to 1024 (the neighbours +-64 and, at d = 384, the
    multiples of 64 between the members among them), kwo = 0 and dh != d / 2 are refused"""
    lib = L.load()
    for kwo in range(0, 1025, 16):
        assert lib.vog_tx_tail_supported(d, d // 2, kwo) == int(kwo in KWO[d]), (d, kwo)
    for kwo in KWO[d]:
        for dh in (d // 2 - 32, d // 2 + 32, d):
            assert lib.vog_tx_tail_supported(d, dh, kwo) == 0, (d, dh, kwo)


def test_head_layouts_map_into_the_rule():
    """the rule is what 1 .. 8 heads give through the head padding (32 / 64 / 128 / 192 / 256 columns per head), 7 heads aside
    (448: not built, such a stack runs the unfused chain)"""
    def pad(c):
        return next(p for p in (32, 64, 128, 192, 256, -1) if c <= p or p < 0)
    for d in KWO:
        got = set()
        for H in range(1, 9):
            dp = pad(-(-d // H))
            if dp > 0 and H != 7:
                got.add(H * dp)
        assert got == set(KWO[d]), (d, got)


def test_default_widths_keep_their_rule():
    lib = L.load()
    for kwo in range(0, 1025, 16):
        assert lib.vog_tx_tail_supported(512, 256, kwo) == int(0 < kwo <= 768 and kwo % 64 == 0), kwo
        assert lib.vog_tx_tail_supported(768, 384, kwo) == int(0 < kwo <= 768 and kwo % 192 == 0), kwo
