"""CPU: the host side of the language bank - which form of the language side a batch dict carries (`engine.language_kind`) and
its messages, the size of a bank row against the shapes, the host logic of `LangBank` (staleness, the refusal to write its
columns by hand), `cfg.hip.lang_bank` and its needs-`query_bank` refusal, the `main_dist --query_bank=lang` arguments."""
import importlib

import pytest
import torch

L = importlib.import_module("vognet-pytorch_amd.lib")
dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
engine_mod = importlib.import_module("vognet-pytorch_amd.engine")
main_dist = importlib.import_module("vognet-pytorch_amd.main_dist")


def test_language_kind_rules_and_messages():
    lk = engine_mod.language_kind
    ARG, WORDS = engine_mod.ARG_KEYS, engine_mod.WORD_KEYS
    assert ARG == ("lang_arg_vec", "lang_final_hidden")
    assert WORDS == ("srl_arg_words_ind", "srl_arg_word_mask", "srl_arg_word_mask_len", "srl_arg_words_capture")
    assert WORDS == engine_mod.NSRL_KEYS_I64[:4] == dls.LangBank.WORD_KEYS and "srl_arg_inds_msk" not in WORDS
    words = dict.fromkeys(WORDS + ("srl_arg_inds_msk", "num_cmp_msk", "pad_proposals"))
    assert lk(words) == "words" and lk({}) == "words"
    assert lk({ARG[0]: 0, "srl_arg_inds_msk": 0}) == "vec"                  # spat / temp: the argument vectors alone
    assert lk({ARG[0]: 0, ARG[1]: 0, "srl_arg_inds_msk": 0}) == "vec"       # sep / svsq: with the final hidden projection
    for k in WORDS:                                                         # a mix, by any one word-level key
        with pytest.raises(ValueError, match="not both"):
            lk({ARG[0]: 0, k: 0})
    with pytest.raises(ValueError, match="not both"):
        lk({**words, ARG[0]: 0, ARG[1]: 0})
    with pytest.raises(ValueError, match="comes with 'lang_arg_vec'"):
        lk({ARG[1]: 0})
    # the language form is independent of the feature form
    assert engine_mod.feature_kind({ARG[0]: 0, "enc_region_feature": 0, "enc_seg_feature": 0}) == "enc"
    assert "fp32 plan" in engine_mod.LANG_F32_RULE and "word-level" in engine_mod.LANG_F32_RULE


def test_bytes_per_query_against_the_shapes():
    bpq = dls.LangBank.bytes_per_query
    # cfg 2 (spat: one sentence per query, 5 arguments, lang_enc 256): 5 KB of argument vectors; with a final hidden row 1 KB more
    assert bpq(5, 256) == 5 * 256 * 4 == 5120
    assert bpq(5, 256, 1, True) == 5120 + 1024
    # sep: one sentence per video
    assert bpq(5, 256, 4, True) == 4 * (5120 + 1024)
    for nsrl, lang_enc, nvl, sep in ((5, 16, 1, False), (3, 32, 4, True), (1, 8, 2, True)):
        vec = torch.zeros(nvl, nsrl, lang_enc)
        fh = torch.zeros(nvl, lang_enc)
        want = vec.numel() * 4 + (fh.numel() * 4 if sep else 0)
        assert bpq(nsrl, lang_enc, nvl, sep) == want
    # against the word-level columns it replaces at cfg 2: [1, 5, 20] + [1, 20] + [1] + [1, 5, 2] int64 = 1,048 B... per sentence
    words = (5 * 20 + 20 + 1 + 5 * 2) * 8
    assert words == 1048 and bpq(5, 256) > words


class _Eng:
    def __init__(self):
        self.weights_epoch, self.plan = 3, "f16"


def _host_lbank():
    b = dls.LangBank.__new__(dls.LangBank)
    b.Q, b.device = 4, torch.device("cpu")
    b.spec = {"lang_arg_vec": ((1, 5, 16), torch.float32), "target_cmp": ((), torch.int64)}
    b.host_keys = ()
    b.tab = {k: torch.zeros((4,) + shp, dtype=dt) for k, (shp, dt) in b.spec.items()}
    b.host = {}
    b._bad = torch.zeros(16, dtype=torch.int32)
    b.engine = _Eng()
    b.epoch, b.plan, b.geometry, b.source = 3, "f16", (4, 12), None
    return b


def test_lang_bank_host_logic():
    assert issubclass(dls.LangBank, dls.QueryBank)
    b = _host_lbank()
    assert not b.stale() and b.lossless_for(b.engine)
    b.check()
    assert b.stale(_Eng())                                                  # another engine
    b.engine.weights_epoch = 4
    assert b.stale() and not b.lossless_for(b.engine)
    with pytest.raises(L.VogError, match="refresh"):
        b.check()
    b.engine.weights_epoch, b.engine.plan = 3, "split"
    with pytest.raises(L.VogError, match="precision plan"):
        b.check()
    b.engine.plan = "f16"
    b.check()
    with pytest.raises(L.VogError, match="kept none"):
        b.refresh()
    for k in ("lang_arg_vec", "lang_final_hidden", "srl_arg_words_ind"):
        with pytest.raises(TypeError, match="encode / refresh"):
            b.put(0, {k: torch.zeros(1)})
    b.put(1, {"target_cmp": torch.tensor([2, 3])})                          # the other columns stay writable
    assert b.tab["target_cmp"].tolist() == [0, 2, 3, 0]
    b._bad[0] = 1
    with pytest.raises(L.VogError, match="outside"):
        b.check()


def test_config_and_cli():
    cfg = ec.get_default_cfg()
    assert cfg.hip.lang_bank is False
    ec.update_from_dict(cfg, {"hip.lang_bank": "True"})
    assert cfg.hip.lang_bank is True
    with pytest.raises(ValueError, match="needs cfg.hip.query_bank"):
        ec.post_proc_config(cfg)
    ec.update_from_dict(cfg, {"hip.query_bank": "True"})
    with pytest.raises(ValueError, match="cfg.hip.val_graph"):
        ec.check_hip_options(cfg)
    ec.update_from_dict(cfg, {"hip.val_graph": "True"})
    assert ec.post_proc_config(cfg) is cfg
    ec.check_hip_options(ec.get_default_cfg())
    uid, kw = main_dist.parse_argv(["exp1", "--feature_bank=f16", "--query_bank=lang", "--only_val"])
    assert kw["query_bank"] == "lang" and kw["feature_bank"] == "f16" and "--query_bank=lang" in main_dist.__doc__
    with pytest.raises(SystemExit, match="--query_bank=lang needs --feature_bank"):
        main_dist.main_dist("exp1", query_bank="lang", only_val="True")
    with pytest.raises(SystemExit, match="one of True, False, lang"):
        main_dist.main_dist("exp1", query_bank="words", feature_bank="f16", only_val="True")
