"""Host side of fine-tuning (no GPU): the C ABI of the grouped optimiser step (vog_opt_step_groups_f32, include/vog_hip.h) and its
argument checks, which run before any launch; parameter-group resolution (`train.resolve_param_groups`,
`trn_utils.params_opt_groups`) on the small/vog_spat model; the rule for cached input forms under frozen stages
(`engine.refuse_cached_forms(..., frozen=)`); `cfg.hip.train_freeze`; and the float64 restatement of Adam with L2 weight decay
that tests/test_gpu_finetune.py compares the kernels with, against torch.optim.Adam itself."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest
import torch

from oracle import cases
from tests.finetune_ref import adam64_groups
from tests.gpu_util import comm_for

L = importlib.import_module("vognet-pytorch_amd.lib")
E = importlib.import_module("vognet-pytorch_amd.engine")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")
trn = importlib.import_module("vognet-pytorch_amd.train")

NAME = "small/vog_spat"
FAKE = 0x10000          # never dereferenced: a faulty call returns before it touches the device


# ---------------------------------------------------------------- ABI
def test_group_structs_match_the_header_and_the_entry_is_built(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang")
    found = [shutil.which(c) for c in ("gcc", "cc", "clang")] + [rocm_clang if os.access(rocm_clang, os.X_OK) else None]
    found = [c for c in found if c]
    assert found, f"no C compiler: none of gcc, cc, clang on PATH and no {rocm_clang}"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"vog_opt_group": L.OptGroup, "vog_opt_groups_args": L.OptGroupsArgs}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vog_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append(f'  printf("{cname} - %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            src.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    src += ['  return 0;', '}']
    cfile = tmp_path / "abi.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.run([found[0], "-I", os.path.join(root, "include"), str(cfile), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        cname, field, val = line.split()
        cls = pairs[cname]
        if field == "-":
            assert C.sizeof(cls) == int(val), (cname, C.sizeof(cls), val)
        else:
            assert getattr(cls, field).offset == int(val), (cname, field, val)
        seen += 1
    assert seen == 2 + 4 + 3
    assert C.sizeof(L.OptGroup) == 16 and L.OptGroupsArgs.base.offset == 0 and L.OptGroupsArgs.base.size == C.sizeof(L.OptArgs)
    lib = L.load()
    assert lib.vog_version() == 1
    assert "vog_opt_step_groups_f32" in L.SYMBOLS and lib.vog_opt_step_groups_f32 is not None
    header = open(os.path.join(root, "include", "vog_hip.h")).read()
    assert "int vog_opt_step_groups_f32(const vog_opt_groups_args* a, void* stream);" in header
    assert "L2" in header and "decoupled" in header         # which form of weight decay it is


def _gargs(groups, n_tensors=6, mode_b=False):
    arr = (L.OptTensor * n_tensors)()
    for i in range(n_tensors):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, 100
    ga = L.OptGroupsArgs()
    a = ga.base
    a.tensors, a.n_tensors = arr, n_tensors
    a.lr, a.beta1, a.beta2, a.eps, a.step = 1e-3, 0.9, 0.99, 1e-8, 1
    if mode_b:
        a.state, a.scratch = FAKE + 0x4000, FAKE + 0x5000
        a.scratch_bytes = int(L.load().vog_opt_scratch_bytes(n_tensors, 100 * n_tensors))
        a.growth_factor, a.backoff_factor, a.growth_interval = 2.0, 0.5, 2000
    garr = (L.OptGroup * max(len(groups), 1))()
    for i, (first, count, lr, wd) in enumerate(groups):
        garr[i].first, garr[i].count, garr[i].lr, garr[i].weight_decay = first, count, lr, wd
    ga.groups, ga.n_groups = garr, len(groups)
    return ga, (arr, garr)


GROUP_FAULTS = {
    "overlap": ([(0, 3, 1e-3, 0.0), (2, 2, 1e-3, 0.0)], b"ascending"),
    "descending": ([(3, 2, 1e-3, 0.0), (0, 2, 1e-3, 0.0)], b"ascending"),
    "empty group": ([(0, 2, 1e-3, 0.0), (3, 0, 1e-3, 0.0)], b"empty"),
    "negative count": ([(0, -1, 1e-3, 0.0)], b"empty"),
    "count past the table": ([(0, 2, 1e-3, 0.0), (4, 3, 1e-3, 0.0)], b"the table has 6"),
    "negative first": ([(-1, 2, 1e-3, 0.0)], b"ascending"),
    "negative lr": ([(0, 2, -1e-3, 0.0)], b"lr"),
    "negative weight decay": ([(0, 2, 1e-3, -0.1)], b"weight_decay"),
    "no groups": ([], b"n_groups"),
}


@pytest.mark.parametrize("mode_b", [False, True])
@pytest.mark.parametrize("fault", sorted(GROUP_FAULTS))
def test_group_argument_errors_come_back_before_any_device_call(fault, mode_b):
    """The pointers are fakes: a call that got as far as a launch (or a device read) would crash, not return."""
    lib = L.load()
    groups, word = GROUP_FAULTS[fault]
    ga, keep = _gargs(groups, mode_b=mode_b)
    assert lib.vog_opt_step_groups_f32(C.byref(ga), None) != 0
    assert word in lib.vog_last_error(), (fault, lib.vog_last_error())


def test_group_entry_checks_covered_tensors_only_and_the_shared_fields():
    lib = L.load()
    assert lib.vog_opt_step_groups_f32(None, None) != 0
    ga, keep = _gargs([(0, 2, 1e-3, 0.0)])
    ga.groups = C.POINTER(L.OptGroup)()
    assert lib.vog_opt_step_groups_f32(C.byref(ga), None) != 0
    # a covered tensor's fault is an error ...
    ga, (arr, garr) = _gargs([(0, 2, 1e-3, 0.0), (4, 2, 1e-3, 0.01)])
    arr[5].g = None
    assert lib.vog_opt_step_groups_f32(C.byref(ga), None) != 0
    ga, keep = _gargs([(0, 2, 1e-3, 0.0)])
    ga.base.beta1 = 1.0
    assert lib.vog_opt_step_groups_f32(C.byref(ga), None) != 0
    ga, keep = _gargs([(0, 2, 1e-3, 0.0)])
    ga.base.step = 0
    assert lib.vog_opt_step_groups_f32(C.byref(ga), None) != 0 and b"step" in lib.vog_last_error()
    ga, keep = _gargs([(0, 6, 1e-3, 0.0)], mode_b=True)
    ga.base.scratch_bytes -= 1
    assert lib.vog_opt_step_groups_f32(C.byref(ga), None) != 0 and b"scratch" in lib.vog_last_error()


# ---------------------------------------------------------------- group resolution
_MODEL = {}


def _model():
    if not _MODEL:
        cfg, sd, batch, c = cases.build(NAME)
        mdl = sel_mod.get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm_for(c))
        _MODEL.update(cfg=cfg, sd=sd, mdl=mdl, names=[k for k in mdl.state_dict()])
    return _MODEL


LANG = ("lstm_encoder.", "lstm_out_feat_proj.", "srl_arg_words_out_enc.")


def test_stage_names_and_prefixes_freeze():
    names = _model()["names"]
    assert E.TRAIN_STAGES == {"lang": LANG, "enc": ("prop_encoder.", "seg_encoder."), "obj": ("obj_txf.", "pe_obj_sub_enc.")}
    groups, frozen = trn.resolve_param_groups(names, None, ("lang",))
    assert groups is None and frozen == {k for k in names if k.startswith(LANG)} and len(frozen) == 21
    _, frozen = trn.resolve_param_groups(names, None, ("enc", "obj", "lin2.0.weight", "mult_txf."))
    want = {k for k in names if k.startswith(("prop_encoder.", "seg_encoder.", "obj_txf.", "pe_obj_sub_enc.", "mult_txf."))}
    assert frozen == want | {"lin2.0.weight"}
    assert trn.resolve_param_groups(names, None, "enc, lang")[1] == trn.resolve_param_groups(names, None, ("enc", "lang"))[1]
    assert trn.resolve_param_groups(names, None, None) == (None, frozenset())
    with pytest.raises(ValueError, match="no_such_stage"):
        trn.resolve_param_groups(names, None, ("no_such_stage",))


def test_param_groups_by_name_and_prefix():
    names = _model()["names"]
    groups, frozen = trn.resolve_param_groups(
        names, [{"params": ["mult_txf.", "lin2."], "lr": 1e-5}, {"params": ["prop_encoder.0.weight"], "weight_decay": 0.01}])
    assert [g["lr"] for g in groups] == [1e-5, None] and [g["weight_decay"] for g in groups] == [0.0, 0.01]
    assert groups[0]["names"] == sorted(k for k in names if k.startswith(("mult_txf.", "lin2.")))
    assert groups[1]["names"] == ["prop_encoder.0.weight"]
    assert frozen == set(names) - set(groups[0]["names"]) - {"prop_encoder.0.weight"}
    # `freeze` also holds inside a group; a group that ends up empty is gone
    groups, frozen = trn.resolve_param_groups(names, [{"params": ["lin2."]}, {"params": ["lstm_encoder."]}], ("lang",))
    assert len(groups) == 1 and groups[0]["names"] == sorted(k for k in names if k.startswith("lin2."))
    assert "lstm_encoder.embed_tokens.weight" in frozen
    # a plain list of names is one group
    groups, _ = trn.resolve_param_groups(names, ["lin2.", "mult_txf."])
    assert len(groups) == 1 and groups[0]["lr"] is None
    # torch's own keys with the trainer's values pass
    trn.resolve_param_groups(names, [{"params": ["lin2."], "betas": (0.9, 0.99), "eps": 1e-8, "amsgrad": False, "maximize": False,
                                      "capturable": False, "foreach": None}])


@pytest.mark.parametrize("groups, word", [
    ([{"params": ["lin2."]}, {"params": ["lin2.0.bias"]}], "lin2.0.bias"),                 # overlap
    ([{"params": ["lin2.", "lin3."]}], "lin3."),                                           # matches nothing
    ([{"params": ["lin2."], "betas": (0.9, 0.999)}], "betas"),
    ([{"params": ["lin2."], "eps": 1e-6}], "eps"),
    ([{"params": ["lin2."], "amsgrad": True}], "amsgrad"),
    ([{"params": ["lin2."], "maximize": True}], "maximize"),
    ([{"params": ["lin2."], "capturable": 1}], "capturable"),
])
def test_param_group_value_errors_name_the_offender(groups, word):
    with pytest.raises(ValueError, match=word):
        trn.resolve_param_groups(_model()["names"], groups)


def test_params_opt_dict_tensors_by_identity():
    m = _model()
    mdl, names = m["mdl"], m["names"]
    named = dict(mdl.named_parameters())
    assert list(named) == names                                 # (every state-dict entry of this model is a parameter)
    picked = [p for n, p in named.items() if n.startswith(("mult_txf.", "lin2."))]
    groups = tu.params_opt_groups(mdl, [{"params": picked, "lr": 1e-5}])
    assert groups == [{"params": [n for n in names if n.startswith(("mult_txf.", "lin2."))], "lr": 1e-5}]
    resolved, frozen = trn.resolve_param_groups(names, groups)
    assert frozen == {n for n in names if not n.startswith(("mult_txf.", "lin2."))}          # everything else
    assert resolved[0]["lr"] == 1e-5 and set(resolved[0]["names"]) == set(names) - frozen
    # an iterable of parameters; names mixed in; a generator
    assert tu.params_opt_groups(mdl, (p for p in picked[:2])) == [{"params": groups[0]["params"][:2]}]
    assert tu.params_opt_groups(mdl, [picked[0], "lin2."]) == [{"params": [groups[0]["params"][0], "lin2."]}]
    assert tu.params_opt_groups(mdl, None) is None
    with pytest.raises(ValueError, match="not one of the model's"):
        tu.params_opt_groups(mdl, [{"params": [picked[0], picked[0].detach().clone()]}])
    with pytest.raises(ValueError, match="not one of the model's"):
        tu.params_opt_groups(mdl, [torch.zeros(3)])
    with pytest.raises(ValueError):
        tu.params_opt_groups(mdl, [{"params": [3.5]}])


# ---------------------------------------------------------------- cached forms under frozen stages
RAW = dict.fromkeys(E.NSRL_KEYS_I64 + E.F32_KEYS, 0)
FORMS = {f.name: f for f in E.INPUT_FORMS}


def _batch(form):
    return {**{k: 0 for k in RAW if k not in form.replaces}, **dict.fromkeys(form.keys, 0)}


def test_input_forms_own_their_stages():
    assert FORMS["enc"].owns == E.TRAIN_STAGES["enc"] and FORMS["vec"].owns == E.TRAIN_STAGES["lang"]
    assert FORMS["obj"].owns == E.TRAIN_STAGES["enc"] + E.TRAIN_STAGES["obj"]


def test_refuse_cached_forms_with_frozen_stages():
    names = _model()["names"]
    vec = _batch(FORMS["vec"])
    # the stage is frozen: silent - by prefix, and by full names with the parameter list
    assert E.refuse_cached_forms(vec, "trainer", frozen=LANG) is None
    assert E.refuse_cached_forms(vec, "trainer", frozen=[k for k in names if k.startswith(LANG)], params=names) is None
    assert E.refuse_cached_forms(_batch(FORMS["enc"]), "trainer", frozen=trn.expand_freeze(names, ("enc",)), params=names) is None
    assert E.refuse_cached_forms(_batch(FORMS["obj"]), "trainer", frozen=("prop_encoder.", "seg_encoder.", "obj_txf.", "pe_obj_sub_enc.")) is None
    # nothing frozen: the unchanged message
    for frozen in ((), None, frozenset()):
        with pytest.raises(L.VogError) as e:
            E.refuse_cached_forms(vec, "trainer", frozen=frozen)
        assert str(e.value) == E._refusal(FORMS["vec"], "trainer") and "trains the language side" in str(e.value)
    with pytest.raises(L.VogError) as e0:
        E.refuse_cached_forms(vec, "trainer")
    assert str(e0.value) == str(e.value)
    # only the BiLSTM frozen: refused, and the message names what is still trained
    with pytest.raises(L.VogError) as e:
        E.refuse_cached_forms(vec, "trainer", frozen=("lstm_encoder.",), params=names)
    msg = str(e.value)
    assert "srl_arg_words_out_enc.0.weight" in msg and "partly frozen" in msg and "lang_arg_vec" in msg
    assert "lstm_out_feat_proj.0.weight is still trained" in msg          # the first one, in state-dict order
    with pytest.raises(L.VogError, match="srl_arg_words_out_enc."):
        E.refuse_cached_forms(vec, "trainer", frozen=("lstm_encoder.", "lstm_out_feat_proj."))
    # obj rows need the encoders AND obj_tx frozen; a frozen language side does not let encoded features through
    with pytest.raises(L.VogError, match="obj_txf."):
        E.refuse_cached_forms(_batch(FORMS["obj"]), "trainer", frozen=trn.expand_freeze(names, ("enc",)), params=names)
    with pytest.raises(L.VogError) as e:
        E.refuse_cached_forms(_batch(FORMS["enc"]), "trainer", frozen=LANG, params=names)
    assert str(e.value) == E._refusal(FORMS["enc"], "trainer")              # (nothing of ITS stage is frozen: today's text)
    # raw batches pass whatever is frozen; the other sites ignore nothing they did not before
    assert E.refuse_cached_forms(dict(RAW), "trainer", frozen=LANG) is None
    with pytest.raises(ValueError, match="pair"):
        E.refuse_cached_forms({**RAW, "enc_seg_feature": 0}, "trainer", frozen=LANG)


# ---------------------------------------------------------------- config
def test_train_freeze_config_key():
    cfg = ec.get_default_cfg()
    assert cfg.hip.train_freeze == "" and tu.train_freeze(cfg) == ()
    uid, kw = main_mod.parse_argv(["run1", "--hip.train_freeze=enc,lang"])
    ec.update_from_dict(cfg, kw)
    assert cfg.hip.train_freeze == "enc,lang" and tu.train_freeze(cfg) == ("enc", "lang")
    ec.check_hip_options(cfg)
    cfg.hip.train_freeze = "enc,foo"
    with pytest.raises(ValueError, match="foo"):
        ec.check_hip_options(cfg)
    with pytest.raises(ValueError, match="foo"):
        ec.post_proc_config(cfg)
    with pytest.raises(ValueError, match="foo"):
        tu.train_freeze(cfg)
    cfg.hip.train_freeze = " obj , enc,obj "
    assert tu.train_freeze(cfg) == ("obj", "enc")
    del cfg["hip"]
    assert tu.train_freeze(cfg) == ()
    assert "--hip.train_freeze" in main_mod.__doc__


# ---------------------------------------------------------------- the weight-decay formula
def test_float64_restatement_equals_torch_adam_with_weight_decay():
    """Three steps on three small tensors in two groups (two learning rates, one group with weight_decay), in float64 on the
    CPU: the restatement the GPU tests use against torch.optim.Adam itself, to 1e-12 relative."""
    gen = torch.Generator().manual_seed(7)
    sizes = (5, 17, 3)
    p0 = [torch.randn(n, generator=gen, dtype=torch.float64) for n in sizes]
    gs = [[torch.randn(n, generator=gen, dtype=torch.float64) for n in sizes] for _ in range(3)]
    b1, b2, eps = 0.9, 0.99, 1e-8
    spans = [(0, 2, 1e-3, 0.01), (2, 1, 3e-4, 0.0)]
    tp = [torch.nn.Parameter(t.clone()) for t in p0]
    opt = torch.optim.Adam([{"params": tp[:2], "lr": 1e-3, "weight_decay": 0.01}, {"params": tp[2:], "lr": 3e-4}], betas=(b1, b2), eps=eps)
    p, m, v = [t.clone() for t in p0], [torch.zeros_like(t) for t in p0], [torch.zeros_like(t) for t in p0]
    for step in (1, 2, 3):
        for t, g in zip(tp, gs[step - 1]):
            t.grad = g.clone()
        opt.step()
        p, m, v, _ = adam64_groups(p, gs[step - 1], m, v, step, spans, b1, b2, eps)
        for i in range(3):
            st = opt.state[tp[i]]
            for got, ref in ((p[i], tp[i].detach()), (m[i], st["exp_avg"]), (v[i], st["exp_avg_sq"])):
                assert float(((got - ref).abs() / ref.abs().clamp(min=1e-300)).max()) <= 1e-12, (step, i)
    assert not torch.equal(p[0], p0[0])
    # with the decay off the same function is plain Adam (and differs from the decayed run)
    q, *_ = adam64_groups(p0, gs[0], [torch.zeros_like(t) for t in p0], [torch.zeros_like(t) for t in p0], 1,
                          [(0, 2, 1e-3, 0.0), (2, 1, 3e-4, 0.0)], b1, b2, eps)
    r, *_ = adam64_groups(p0, gs[0], [torch.zeros_like(t) for t in p0], [torch.zeros_like(t) for t in p0], 1, spans, b1, b2, eps)
    assert torch.equal(q[2], r[2]) and not torch.equal(q[0], r[0])
