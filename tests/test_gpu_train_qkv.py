"""The factored Q / K / V projections of mul_tx's layer 0 on the device (`vog_attn_f32_vl`, `vog_attn_fused_f32_vl`; the kernels
vl_expand_kernel, vl_reduce_kernel, vl_reduce_groups_kernel in csrc/train_tx.hip): against CPU autograd through `_attn_ref` on
the concatenated tokens, against the dense entries between `vog_conc_f32_fwd` and `vog_conc_f32_bwd` (also under dropout),
bit-reproducibility, `accumulate`, every subset of outputs, the rounded restatement under amp, the launch counter, and through
the trainer / autograd path with `qkv="factored"`. Every operator call runs with BOTH scratch buffers - the operator's and the
descriptor's - at exactly their declared size between two guard bands, at both shifts of the base."""
import contextlib
import functools
import importlib
import itertools
import math

import numpy as np
import pytest
import torch

from tests import qkv_ref as Q
from tests.test_gpu_amp import _ACC, _RMM, _check, _switch, MODES
from tests.test_gpu_bwd_ops import _attn_ref
from tests.test_gpu_train_attn import SHIFTS, TOL, TOL_SUM, close
from tests.test_gpu_train_ops import guarded

pytestmark = pytest.mark.gpu
bwd = importlib.import_module("vognet-pytorch_amd.backward")
L = bwd.L
OPS = ("materialized", "fused", "fused_pipe")
OUT = ("g_wq", "g_wk", "g_wv", "g_pe_w", "g_pe_b", "d_ps", "d_lang")
SUMS = ("g_pe_w", "g_pe_b", "d_lang")              # the long sums: TOL_SUM
CASES = [(s, m) for s in Q.SHAPES for m in (False, True)]
IDS = ["x".join(map(str, s[:8])) + ("-masked" if m else "") for s, m in CASES]


@functools.lru_cache(maxsize=None)
def _ref(shape, masked):
    """CPU autograd in fp32 through `_attn_ref` on the concatenated tokens: computed once per case, read-only."""
    return Q.dense(Q.case(shape, masked), torch.float32, attn=_attn_ref)


def _dev(c, **want):
    w = {"wq": c["ws"][0].cuda(), "wk": c["ws"][1].cuda(), "wv": c["ws"][2].cuda()}
    boxes = bwd._Boxes(c["props"].cuda(), Q.VW, Q.VH, float(c["nfrm"])) if c["rel"] else None
    pe = (c["pe_w"].cuda(), c["pe_b"].cuda()) if c["rel"] else None
    n_q, nc_v, nfrm, n, nsrl, _, _, lpv = c["shape"][:8]
    vl = bwd.FactoredInput(c["ps"].cuda(), c["lang"].cuda(), c["msk"].cuda() if c["msk"] is not None else None, n_q, nc_v, nfrm, n,
                           nsrl, lang_per_vid=bool(lpv), **want)
    dc = c["d_cat"].reshape(c["S"] * c["N"], c["d"]).cuda().contiguous()
    return (w, pe, None, c["S"], c["N"], n, c["H"], boxes), vl, dc


@contextlib.contextmanager
def _pipe(on):
    lib = L.load()
    assert lib.vog_train_set_int(b"attn_fused_pipe", 1 if on else 0) == 0
    try:
        yield
    finally:
        lib.vog_train_set_int(b"attn_fused_pipe", 0)


def vl_call(args, vl, op="materialized", shift=1, **kw):
    """One `_vl` call with both scratch buffers guarded at `shift`."""
    lib = L.load()
    S, N, n, H = args[3], args[4], args[5], args[6]
    d = vl.dobj + vl.dlang
    fused = op != "materialized"
    nb = lib.vog_attn_fused_scratch_bytes(S, N, n, d, H) if fused else lib.vog_attn_f32_scratch_bytes(S, N, n, d)
    with guarded(nb, 8, shift) as sc, guarded(lib.vog_attn_vl_scratch_bytes(*vl.geometry()), 0, shift) as vsc, _pipe(op == "fused_pipe"):
        return bwd._attn_call(*args, scratch=sc, vl=vl, vl_scratch=vsc, **({"fused": True} if fused else {}), **kw)


def _tol(k):
    return TOL_SUM if k in SUMS else TOL


def _close_all(got, ref, op):
    """Every output against `ref` at the bounds of tests/test_gpu_train_attn.py, relative to the reference's largest entry.
    With ONE key the softmax's Jacobian vanishes: dS = P (dP - sum P dP) is exactly 0 in the reference, so g_wq, g_wk and g_pe_*
    are identically zero, while the fused kernels form the same difference from a delta and a dP that were each rounded (under
    dropout they no longer cancel to the last bit). A relative measure has no scale there; the error is then taken relative to
    the quantity of the same kind that does not cancel, the largest reference entry of g_wv = dV^T x."""
    for k in OUT:
        if ref.get(k) is None:
            continue
        r = ref[k]
        if float(r.abs().max()) == 0.0 and k in ("g_wq", "g_wk", "g_pe_w", "g_pe_b"):
            err = float(got[k].detach().cpu().double().abs().max()) / float(ref["g_wv"].abs().max())
            print(f"    {op} {k}: reference identically zero, {err:.3e} of g_wv's largest entry (bound {_tol(k):.0e})")
            assert err <= _tol(k), (op, k, err)
        else:
            close(got[k], r, tol=_tol(k), what=f"{op} {k}")


# ---------------------------------------------------------------- fp32 against CPU autograd
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("shape,masked", CASES, ids=IDS)
def test_vl_f32_vs_cpu_autograd(shape, masked, shift):
    c, ref = Q.case(shape, masked), _ref(shape, masked)
    args, vl, dc = _dev(c)
    for op in OPS:
        f = vl_call(args, vl, op, shift)
        r = vl_call(args, vl, op, shift, d_cat=dc, want_cat=True)
        torch.cuda.synchronize()
        close(f["cat"], ref["cat"], what=f"{op} cat")
        close(r["cat"], ref["cat"], what=f"{op} cat of the backward call")
        _close_all(r, ref, op)
        if masked:                                                        # a masked argument row gets an exactly-zero gradient
            assert float(r["d_lang"][~c["msk"].bool().cuda()].abs().max()) == 0.0


# ---------------------------------------------------------------- device against device: the dense entries between the conc kernels
def _dense_on_device(c, fused, drop, dc):
    lib, st = L.load(), L.stream_ptr()
    n_q, nc_v, nfrm, n, nsrl, dobj, dlang, lpv = c["shape"][:8]
    args, vl, _ = _dev(c)
    x = torch.empty(c["S"] * c["N"], c["d"], dtype=torch.float32, device="cuda")
    L.check(lib.vog_conc_f32_fwd(L.ptr(vl.ps), L.ptr(vl.lang), L.ptr(vl.msk), L.ptr(x), n_q, nc_v, nfrm, n, nsrl, dobj, dlang, lpv, st),
            "vog_conc_f32_fwd")
    a = (args[0], args[1], x) + args[3:]
    kw = {"fused": True} if fused else {}
    f = bwd._attn_call(*a, drop=drop, **kw)
    r = bwd._attn_call(*a, d_cat=dc, drop=drop, **kw)
    r["d_ps"], r["d_lang"] = bwd.conc_backward(r["d_x"], n_q, nc_v, nfrm, n, nsrl, dobj, inds_msk=vl.msk, lang_per_vid=bool(lpv))
    return f, r


@pytest.mark.parametrize("drop", [None, (0.2, 77, 210)], ids=["eval", "dropout"])
@pytest.mark.parametrize("shape,masked", CASES, ids=IDS)
def test_vl_vs_dense_entry_on_the_device(shape, masked, drop):
    """Same inputs, same dropout masks (element index and site do not depend on where q, k, v come from)."""
    c = Q.case(shape, masked)
    args, vl, dc = _dev(c)
    for op in OPS:
        df, dr = _dense_on_device(c, op != "materialized", drop, dc)
        f = vl_call(args, vl, op, 252, drop=drop)
        r = vl_call(args, vl, op, 1, d_cat=dc, drop=drop)
        torch.cuda.synchronize()
        close(f["cat"], df["cat"], what=f"{op} cat")
        _close_all(r, dr, op)


# ---------------------------------------------------------------- the same bits on every run; accumulate
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("idx", [2, 3, 6, 7, 8])
def test_two_calls_give_the_same_bits_and_accumulate_adds(idx, op):
    c = Q.case(Q.SHAPES[idx], True)
    args, vl, dc = _dev(c)
    a = vl_call(args, vl, op, 1, d_cat=dc, want_cat=True, drop=(0.2, 77, 210))
    b = vl_call(args, vl, op, 252, d_cat=dc, want_cat=True, drop=(0.2, 77, 210))
    torch.cuda.synchronize()
    for k in ("cat",) + OUT:
        if k in a:
            assert torch.equal(a[k], b[k]), k
    full = vl_call(args, vl, op, 1, d_cat=dc)
    g = torch.Generator().manual_seed(5)
    base = {"d_ps": torch.randn(vl.ps.shape, generator=g).cuda(), "d_lang": torch.randn(vl.lang.shape, generator=g).cuda()}
    r = vl_call(args, vl, op, 1, d_cat=dc, d_ps=base["d_ps"].clone(), d_lang=base["d_lang"].clone(), accumulate_dx=True)
    torch.cuda.synchronize()
    for k in ("d_ps", "d_lang"):
        # base + p1 + p2 + p3 against (p1 + p2 + p3) summed first, then one rounding of the final sum: three fp32 additions on
        # either side, each within half a unit (2^-24) of the result's size - tests/test_gpu_train_attn.py::test_options
        want = base[k].double() + full[k].double()
        close(r[k], want, tol=6 * 2.0 ** -24, what=f"accumulated {k}")
    for k in ("g_wq", "g_wk", "g_wv"):
        assert torch.equal(r[k], full[k]), k


# ---------------------------------------------------------------- every subset of the outputs
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("idx", [1, 8])
def test_every_subset_of_outputs(idx, op):
    """The present outputs carry the full call's bits; an absent one has no buffer (NULL), and both guard bands hold."""
    c = Q.case(Q.SHAPES[idx], True)
    full_args, full_vl, dc = _dev(c)
    full = vl_call(full_args, full_vl, op, 1, d_cat=dc)
    names = ("wq", "wk", "wv", "pe", "d_ps", "d_lang")
    keys = {"wq": ["g_wq"], "wk": ["g_wk"], "wv": ["g_wv"], "pe": ["g_pe_w", "g_pe_b"], "d_ps": ["d_ps"], "d_lang": ["d_lang"]}
    for mask in itertools.product((False, True), repeat=len(names)):
        sub = {n for n, on in zip(names, mask) if on}
        args, vl, _ = _dev(c, want_ps="d_ps" in sub, want_lang="d_lang" in sub)
        r = vl_call(args, vl, op, 252, d_cat=dc, want=sub & {"wq", "wk", "wv", "pe"}, want_dx=bool(sub & {"d_ps", "d_lang"}))
        torch.cuda.synchronize()
        for n in names:
            for k in keys[n]:
                if n in sub:
                    assert torch.equal(r[k], full[k]), (sorted(sub), k)
                else:
                    assert k not in r, (sorted(sub), k)


# ---------------------------------------------------------------- amp: the rounded restatement
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("idx,masked", [(1, True), (3, False), (5, True), (7, False)])
def test_vl_amp_vs_rounded_restatement(idx, masked, mode):
    """The restatement rounds where the factored operator rounds: ps, mask * lang and the weights' column blocks in the
    projections, the summed dPv / dPl in the gradient products; q, k, v, P, dO, dS in the attention as `_attn_rounded` does."""
    dt, amp = MODES[mode]
    c = Q.case(Q.SHAPES[idx], masked)
    rmm = lambda a, b: _RMM.apply(a, b, dt)
    ref = Q.factored(c, torch.float32, P=rmm, mm=rmm)
    _ACC[0] = torch.float64
    try:
        alt = Q.factored(c, torch.float32, P=rmm, mm=rmm)
    finally:
        _ACC[0] = torch.float32
    args, vl, dc = _dev(c)
    lib = L.load()
    for op in ("materialized", "fused"):
        assert lib.vog_train_set_int(b"amp", amp) == 0 and lib.vog_train_set_int(b"f32_products", 0) == 0
        try:
            f = vl_call(args, vl, op, 1)
            r = vl_call(args, vl, op, 252, d_cat=dc)
            torch.cuda.synchronize()
            assert _switch(b"f32_products") == 0                       # every product of the factored form took 16-bit operands
        finally:
            lib.vog_train_set_int(b"amp", 0)
        case = f"qkv factored {op} {'x'.join(map(str, c['shape'][:8]))}"
        _check(mode, f["cat"], ref["cat"], alt["cat"], f"{case} cat")
        for k in OUT:
            if ref[k] is not None:
                _check(mode, r[k], ref[k], alt[k], f"{case} {k}")


# ---------------------------------------------------------------- the counter
def test_counter_counts_the_new_kernels_only():
    c = Q.case(Q.SHAPES[1], True)
    args, vl, dc = _dev(c)
    lib = L.load()
    for op in OPS:
        assert lib.vog_train_set_int(b"attn_vl_launches", 0) == 0
        _dense_on_device(c, op != "materialized", None, dc)
        assert _switch(b"attn_vl_launches") == 0
        vl_call(args, vl, op, 1)
        assert _switch(b"attn_vl_launches") == 1                        # the forward: vl_expand
        vl_call(args, vl, op, 1, d_cat=dc)
        assert _switch(b"attn_vl_launches") == 4                        # + expand, reduce, reduce_groups
        assert _switch(b"attn_fused_pipe") == 0 and _switch(b"amp") == 0
    assert lib.vog_train_set_int(b"attn_vl_launches", 0) == 0


# ---------------------------------------------------------------- the whole path: trainer, autograd, frozen stages
from tests.gpu_util import comm_for                                         # noqa: E402
from tests.test_gpu_amp import _sd                                          # noqa: E402
from tests.test_gpu_autograd import _build, _close, _grads                  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
cases = importlib.import_module("oracle.cases")
mgb = importlib.import_module("oracle.make_golden_bwd")


@pytest.mark.parametrize("attn", ["materialized", "fused_pipe"])
@pytest.mark.parametrize("name", ["small/vog_spat", "small/vog_sep_cmpmsk", "small/vog_temp", "small/vog_spat_3layers"])
def test_trainer_factored_vs_reference_golden(name, attn):
    """Bounds: tests/test_gpu_train_lstm.py::test_trainer_fused_vs_reference_golden's (loss 2e-5, mdl_outs 1e-4, gradients 5e-3
    of the largest reference entry); the full set of parameter gradients."""
    from tests.test_bwd_oracle import check_fixture
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    lib = L.load()
    tf = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, qkv="factored", attn=attn)
    assert tf.qkv == "factored" and lib.vog_train_set_int(b"attn_vl_launches", 0) == 0
    g = np.load(mgb.bwd_path(name))
    lf, gf = tf.gradients(dev)
    assert _switch(b"attn_vl_launches") == 4                                # layer 0's forward and backward, no other layer
    assert _switch(b"attn_fused_pipe") == 0 and _switch(b"amp") == 0       # the switches are reset behind the step
    assert abs(float(lf["loss"]) - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    ref_outs = torch.from_numpy(np.load(cases.golden_path(name))["mdl_outs"])
    outs = tf.forward(dev)[0]["mdl_outs"].cpu()
    assert float((outs - ref_outs).abs().max()) <= 1e-4 * float(ref_outs.abs().max())
    worst = max(check_fixture(g, "p:" + k, v.cpu().numpy(), tol=5e-3) for k, v in gf.items())
    assert len(gf) == sum(1 for k in g.files if k.startswith("p:") and k.endswith("__shape"))
    print(f"    {name} {attn}: worst against the golden {worst:.3e}")


@pytest.mark.parametrize("name", ["small/vog_spat", "full/cfg2_vog_spat_gt5_bs4"])
def test_three_adam_steps_follow_the_default_trainer(name):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    lib = L.load()
    tf = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, qkv="factored")
    td = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    assert td.qkv == "dense"
    a = [float(tf.step(dev)["loss"]) for _ in range(3)]
    assert _switch(b"attn_vl_launches") > 0 and lib.vog_train_set_int(b"attn_vl_launches", 0) == 0
    b = [float(td.step(dev)["loss"]) for _ in range(3)]
    assert _switch(b"attn_vl_launches") == 0                                # the default step touches none of the new kernels
    print("    losses factored", a, "default", b)
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-5 * abs(y), (a, b)


def test_three_adam_steps_in_amp_bf16_track_the_fp32_default():
    """tests/test_gpu_amp.py::test_adam_steps_under_autocast_bf16_track_fp32's bound: 1e-2 of the fp32 loss, and the loss falls.
    The amp step as the record measures it: lstm_amp="split", gemm_amp="pipe", attn="fused_pipe"."""
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build("small/vog_spat")
    tf = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, qkv="factored", amp="bf16", lstm_amp="split", gemm_amp="pipe",
                         attn="fused_pipe")
    td = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4)
    L.load().vog_train_set_int(b"f32_products", 0)
    b = [float(tf.step(dev)["loss"]) for _ in range(3)]
    assert _switch(b"f32_products") == 0
    for nm in (b"amp", b"gemm_amp_pipe", b"attn_fused_pipe", b"lstm_amp_split"):
        assert _switch(nm) == 0, nm
    a = [float(td.step(dev)["loss"]) for _ in range(3)]
    print("    losses fp32 default", a, "factored bf16", b)
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-2 * abs(x), (a, b)
    assert b[-1] < b[0]


def test_autograd_path_takes_the_option_from_the_cfg(monkeypatch):
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    cfg.hip.train_qkv = "factored"
    calls = []
    orig = bwd._attn_call
    monkeypatch.setattr(bwd, "_attn_call", lambda *a, **k: (calls.append(k.get("vl") is not None), orig(*a, **k))[1])
    tr = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, qkv="factored")
    _, ref = tr.gradients(dev)
    n_tr = len(calls)
    assert any(calls) and not all(calls)                         # layer 0 of mul_tx, and only it
    mdl.eval().requires_grad_(True)
    loss_fn(mdl(dev), dev)["loss"].backward()
    assert sum(calls[n_tr:]) == sum(calls[:n_tr])                 # the autograd path: as many calls on the factors
    got = _grads(mdl)
    assert set(got) == set(ref)
    for k, v in ref.items():
        _close(got[k], v.cpu(), 1e-6, k)


@pytest.mark.parametrize("freeze", ["enc,obj", "lang"])
def test_frozen_stages(freeze):
    """want_ps / want_lang = False reach the operator as NULL outputs: the step runs, the frozen stages have no gradient, and
    the trained ones equal the dense trainer's within the fp32 bound of another summation order (2e-5 of the largest entry)."""
    name = "small/vog_spat"
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(name)
    tf = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, qkv="factored", freeze=freeze)
    td = trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, freeze=freeze)
    seen = []
    orig = bwd._attn_call

    def spy(*a, **k):
        r = orig(*a, **k)
        if k.get("vl") is not None and k.get("d_cat") is not None:
            seen.append(("d_ps" in r, "d_lang" in r))
        return r

    bwd._attn_call = spy
    try:
        lf, gf = tf.gradients(dev)
    finally:
        bwd._attn_call = orig
    ld, gd = td.gradients(dev)
    assert seen == [(freeze == "lang", freeze != "lang")], seen
    pre = tuple(p for s in freeze.split(",") for p in trn.TRAIN_STAGES[s])
    assert set(gf) == set(gd) and gf and not any(k.startswith(pre) for k in gf)
    assert abs(float(lf["loss"]) - float(ld["loss"])) <= 2e-5 * abs(float(ld["loss"]))
    worst = max(_close(gf[k], gd[k].cpu(), 2e-5, k) for k in gd)
    print(f"    freeze={freeze}: {len(gf)} gradients, worst against the dense trainer {worst:.3e}")
    assert math.isfinite(float(tf.step(dev)["loss"]))
