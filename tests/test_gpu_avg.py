"""-m gpu: weight averaging behind the optimiser step (vog_opt_average_f32, csrc/optim.hip) and what is wired to it -
`FP32Trainer(avg=)`, the Learner with `cfg.hip.train_avg` / `train_avg_eval`, its checkpoints, two ranks.

The tensor set is test_gpu_opt's SIZES (79 tensors, 1 to 300 001 elements: three launch tables, many chunks, heads and tails);
the last two pairs sit off the 16-byte grid - (avg, p) one element in each (a scalar head, 16-byte groups, a tail) and one / two
elements in (no common alignment: one element per lane). Every avg and p view lies in a buffer whose other elements hold GUARD.

The reference is torch.optim.swa_utils.AveragedModel on float64 copies. Bound per element after update k:
|dev - ref| <= k * 2^-23 * M_k, M_k the running maximum over updates <= k of max(|p|, |ref avg|): one rounding of p - avg and one
of the fused multiply-add per update, and earlier errors never grow since 0 <= 1 - w <= 1."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn, get_swa_multi_avg_fn

from tests.gpu_util import comm_for
from tests.test_gpu_autograd import _build
from tests.test_gpu_dist import _free_port, _rank_batch, _setup
from tests.test_gpu_opt import NAME, SIZES, _read, _sd, _state
from tests.test_gpu_opt_variants import GUARD, _devx, _ex_step, _guards_intact

pytestmark = pytest.mark.gpu

trn = importlib.import_module("vognet-pytorch_amd.train")
L = importlib.import_module("vognet-pytorch_amd.lib")
tu = importlib.import_module("vognet-pytorch_amd.trn_utils")

N_UPD = 8
AOFF = [0] * (len(SIZES) - 2) + [1, 1]          # elements into the buffer: avg
POFF = [0] * (len(SIZES) - 2) + [1, 2]          # ... and p: the last pair disagrees, the one before agrees one element in
HEAD, SCALAR = len(SIZES) - 2, len(SIZES) - 1
CASES = {"ema 0.9": ("ema", 0.9, False), "ema 0.999": ("ema", 0.999, False), "ema 0.999 warm-up": ("ema", 0.999, True),
         "swa": ("swa", 0.0, False)}
SEQS = ("independent", "walk")
OUT_KEYS = ("mdl_outs", "mdl_outs_eval", "_pred_rec")


def _avg_state(n_averaged=0):
    return torch.tensor([n_averaged, 0, 0, 0], dtype=torch.int32).cuda()


def _read_avg(state):
    return L.OptAvgState.from_buffer_copy(state.cpu().numpy().tobytes())


def _average(avg, p, state, mode, decay=0.999, warmup=False, start=1, every=1, step=None, opt_state=None):
    arr = (L.OptAvgTensor * len(avg))()
    for i in range(len(avg)):
        arr[i].avg, arr[i].p, arr[i].n = L.ptr(avg[i]), L.ptr(p[i]), avg[i].numel()
    a = L.OptAvgArgs()
    a.tensors, a.n_tensors = arr, len(avg)
    a.mode, a.decay, a.warmup, a.start, a.every = trn.AVG_MODES[mode], decay, int(warmup), start, every
    if opt_state is not None:
        a.opt_state = L.ptr(opt_state)
    else:
        a.step = step
    a.state = L.ptr(state)
    L.check(L.load().vog_opt_average_f32(C.byref(a), L.stream_ptr()), "vog_opt_average_f32")
    torch.cuda.synchronize()


_SEQ = {}


def _sequence(kind):
    """N_UPD parameter sets on the host (fp32, one flat vector each), made once and never written to."""
    if kind not in _SEQ:
        gen = torch.Generator().manual_seed(4321 if kind == "walk" else 8765)
        total = sum(SIZES)
        if kind == "independent":
            _SEQ[kind] = [torch.randn(total, generator=gen) for _ in range(N_UPD)]
        else:
            out = [torch.randn(total, generator=gen)]
            for _ in range(N_UPD - 1):
                out.append(out[-1] + 1e-3 * torch.randn(total, generator=gen))
            _SEQ[kind] = out
    return _SEQ[kind]


def _split(flat):
    return list(torch.split(flat, SIZES))


class _Holder(torch.nn.Module):
    def __init__(self, ts):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.double().clone(), requires_grad=False) for t in ts])


_REF = {}


def _reference(case, kind):
    """The float64 averages after every update (flat vectors), computed once: AveragedModel, or for the warm-up case the float64
    recurrence avg += (1 - min(decay, (1 + n) / (10 + n))) * (p - avg), the first update a copy."""
    if (case, kind) not in _REF:
        mode, decay, warm = CASES[case]
        seq, out = _sequence(kind), []
        if warm:
            avg = None
            for n, p in enumerate(seq):
                p64 = p.double()
                avg = p64.clone() if n == 0 else avg + (1.0 - min(decay, (1.0 + n) / (10.0 + n))) * (p64 - avg)
                out.append(avg.clone())
        else:
            model = _Holder(_split(seq[0]))
            am = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay) if mode == "ema" else get_swa_multi_avg_fn())
            for p in seq:
                with torch.no_grad():
                    for dst, src in zip(model.ps, _split(p)):
                        dst.copy_(src.double())
                am.update_parameters(model)
                out.append(torch.cat([q.detach().reshape(-1) for q in am.module.ps]).clone())
            assert int(am.n_averaged) == N_UPD
        _REF[(case, kind)] = out
    return _REF[(case, kind)]


def _run(case, kind):
    """The N_UPD updates on the device, mode A -> (avg after every update as flat host vectors, final state, guards intact,
    p untouched)."""
    mode, decay, warm = CASES[case]
    seq = _sequence(kind)
    avg, abufs = _devx([torch.zeros(n) for n in SIZES], AOFF)
    p, pbufs = _devx(_split(seq[0]), POFF)
    assert avg[HEAD].data_ptr() % 16 == 4 and p[HEAD].data_ptr() % 16 == 4
    assert avg[SCALAR].data_ptr() % 16 == 4 and p[SCALAR].data_ptr() % 16 == 8
    st = _avg_state()
    snaps, p_ok = [], True
    for k, flat in enumerate(seq, start=1):
        for dst, src in zip(p, _split(flat)):
            dst.copy_(src)
        _average(avg, p, st, mode, decay=decay, warmup=warm, step=k)
        snaps.append(torch.cat(avg).cpu())
        p_ok = p_ok and torch.equal(torch.cat(p).cpu(), flat)
    return snaps, _read_avg(st), _guards_intact(abufs, AOFF) and _guards_intact(pbufs, POFF), p_ok


_RUNS = {}


def _cached_run(case, kind):
    if (case, kind) not in _RUNS:
        _RUNS[(case, kind)] = _run(case, kind)
    return _RUNS[(case, kind)]


def _worst_ratio(snaps, refs, seq):
    """max over updates and elements of |dev - ref| / (k * 2^-23 * M_k)."""
    worst, M = 0.0, torch.zeros(sum(SIZES), dtype=torch.float64)
    for k, (dev, ref, p) in enumerate(zip(snaps, refs, seq), start=1):
        M = torch.maximum(M, torch.maximum(p.double().abs(), ref.abs()))
        bound = k * 2.0 ** -23 * M
        err = (dev.double() - ref).abs()
        assert bool((bound > 0).all())
        worst = max(worst, float((err / bound).max()))
    return worst


# ---------------------------------------------------------------- 1: values, C ABI, mode A
@pytest.mark.parametrize("kind", SEQS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_eight_updates_against_torchs_averaged_model_in_float64(case, kind):
    snaps, st, guards, p_ok = _cached_run(case, kind)
    worst = _worst_ratio(snaps, _reference(case, kind), _sequence(kind))
    print(f"{case}, {kind}: worst error / bound {worst:.3f}; n_averaged {st.n_averaged}, last w {st.w}")
    assert worst <= 1.0, worst
    assert st.n_averaged == N_UPD and st.updated == 1
    mode, decay, warm = CASES[case]
    n = N_UPD - 1
    want_w = 1.0 / (n + 1) if mode == "swa" else 1.0 - (min(decay, (1.0 + n) / (10.0 + n)) if warm else decay)
    assert st.w == float(np.float32(want_w)), (st.w, want_w)            # formed in double, rounded once


# ---------------------------------------------------------------- 2: cut and alignment
@pytest.mark.parametrize("case", ["ema 0.9", "swa"])
def test_misaligned_pairs_stay_inside_their_tensors_and_p_is_never_written(case):
    snaps, st, guards, p_ok = _cached_run(case, "independent")
    assert guards, "an element next to a tensor was written"
    assert p_ok, "p was written"
    # the two pairs off the 16-byte grid obey the bound on their own (the scalar path, and head + groups + tail)
    refs, seq = _reference(case, "independent"), _sequence("independent")
    for t in (HEAD, SCALAR):
        lo = sum(SIZES[:t])
        sl = slice(lo, lo + SIZES[t])
        M = torch.zeros(SIZES[t], dtype=torch.float64)
        for k in range(1, N_UPD + 1):
            M = torch.maximum(M, torch.maximum(seq[k - 1][sl].double().abs(), refs[k - 1][sl].abs()))
            assert bool(((snaps[k - 1][sl].double() - refs[k - 1][sl]).abs() <= k * 2.0 ** -23 * M).all()), (t, k)
        assert not torch.equal(snaps[0][sl], snaps[-1][sl])


# ---------------------------------------------------------------- 3: the first update is a copy
@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_first_update_copies_the_bits(mode):
    p_host = _split(_sequence("independent")[0].clone())
    for t in p_host:                                            # bit patterns an arithmetic path would not keep
        t[0] = -0.0
        if t.numel() > 6:
            t[5], t[6] = float("inf"), 1e-42
    avg, abufs = _devx([torch.full((n,), 3.0) for n in SIZES], AOFF)
    p, pbufs = _devx(p_host, POFF)
    st = _avg_state()
    _average(avg, p, st, mode, decay=0.5, step=1)
    s = _read_avg(st)
    assert (s.n_averaged, s.updated, s.w) == (1, 1, 1.0)
    for i in range(len(SIZES)):
        assert torch.equal(avg[i].view(torch.int32), p[i].view(torch.int32)), (i, SIZES[i])
        assert torch.equal(p[i].cpu().view(torch.int32), p_host[i].view(torch.int32)), i
    assert _guards_intact(abufs, AOFF) and _guards_intact(pbufs, POFF)


# ---------------------------------------------------------------- 4: schedule
def test_schedule_averages_on_the_chosen_steps_only():
    seq = _sequence("independent")
    avg, abufs = _devx([torch.zeros(n) for n in SIZES], AOFF)
    p, _ = _devx(_split(seq[0]), POFF)
    st = _avg_state()
    n = 0
    for step in range(1, 7):
        for dst, src in zip(p, _split(seq[step - 1])):
            dst.copy_(src)
        before = torch.cat(avg).clone()
        _average(avg, p, st, "swa", start=2, every=2, step=step)
        s = _read_avg(st)
        after = torch.cat(avg)
        if step in (2, 4, 6):
            n += 1
            assert (s.n_averaged, s.updated) == (n, 1) and s.w == float(np.float32(1.0 / n)), (step, s.n_averaged, s.w)
            assert not torch.equal(before, after), step
        else:
            assert (s.n_averaged, s.updated, s.w) == (n, 0, 0.0), (step, s.n_averaged, s.updated, s.w)
            assert torch.equal(before.view(torch.int32), after.view(torch.int32)), step
    assert n == 3 and _guards_intact(abufs, AOFF)
    # the equal-weight mean of the parameters of steps 2, 4, 6
    want = (seq[1].double() + seq[3].double() + seq[5].double()) / 3.0
    M = torch.stack([seq[1], seq[3], seq[5]]).abs().max(0).values.double()
    assert bool(((torch.cat(avg).cpu().double() - want).abs() <= 3 * 2.0 ** -23 * M).all())


# ---------------------------------------------------------------- 5: mode B
def test_mode_b_follows_the_optimisers_decision_and_applied_step_count():
    """A real vog_opt_step_ex_f32 (AdamW, mode B) in front of every averaging call; start = 1, every = 2:
    call 1 clean (adam_step 1: averages, a copy), call 2 with an infinite gradient (skipped: adam_step stays 1, which the schedule
    alone would average AGAIN), call 3 clean (adam_step 2: off the schedule, though it is the third call), call 4 clean
    (adam_step 3: averages with n = 1)."""
    gen = torch.Generator().manual_seed(99)
    p, _ = _devx([torch.randn(n, generator=gen) for n in SIZES], POFF)
    g_host = [torch.randn(n, generator=gen) for n in SIZES]
    m, v = [torch.zeros(n, device="cuda") for n in SIZES], [torch.zeros(n, device="cuda") for n in SIZES]
    avg, abufs = _devx([torch.zeros(n) for n in SIZES], AOFF)
    ost, st = _state(scale=1.0), _avg_state()
    groups = [(0, len(SIZES), 1e-2, 0.01)]

    def both(bad=False):
        g = [t.cuda() for t in g_host]
        if bad:
            g[SCALAR][-1] = float("inf")
        _ex_step(p, g, m, v, groups=groups, flags=L.OPT_DECOUPLED, state=ost, growth=(2.0, 0.5, 0))
        _average(avg, p, st, "swa", start=1, every=2, opt_state=ost)
        return _read(ost), _read_avg(st)

    o, s = both()
    assert (o.adam_step, o.found_inf) == (1, 0) and (s.n_averaged, s.updated, s.w) == (1, 1, 1.0)
    assert all(torch.equal(a, q) for a, q in zip(avg, p))
    first = torch.cat(avg).clone()
    o, s = both(bad=True)
    assert (o.adam_step, o.found_inf, o.skipped) == (1, 1, 1) and (s.n_averaged, s.updated, s.w) == (1, 0, 0.0)
    assert torch.equal(torch.cat(avg), first)
    o, s = both()
    assert (o.adam_step, o.found_inf) == (2, 0) and (s.n_averaged, s.updated, s.w) == (1, 0, 0.0)
    assert torch.equal(torch.cat(avg), first) and not torch.equal(torch.cat(p), first)
    o, s = both()
    assert (o.adam_step, o.found_inf) == (3, 0) and (s.n_averaged, s.updated, s.w) == (2, 1, 0.5)
    want = (first.double() + torch.cat(p).double()) / 2.0
    M = torch.maximum(first.abs(), torch.cat(p).abs()).double()
    assert bool(((torch.cat(avg).double() - want).abs() <= 2 * 2.0 ** -23 * M).all())
    assert _guards_intact(abufs, AOFF)


# ---------------------------------------------------------------- 6: determinism
def test_two_runs_end_with_equal_bits():
    a, sa, _, _ = _cached_run("ema 0.999 warm-up", "walk")
    b, sb, _, _ = _run("ema 0.999 warm-up", "walk")
    assert bytes(sa) == bytes(sb)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------- 7: trainer
def _trainer(built, **kw):
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = built
    return trn.FP32Trainer(cfg, comm_for(c), _sd(sd), loss_fn, lr=1e-4, **kw)


def _ema64(snaps, decay):
    """The float64 recurrence over parameter snapshots -> (averages after the last one, the bound's M)."""
    avg, M = None, None
    for n, p in enumerate(snaps):
        p64 = p.double()
        avg = p64.clone() if n == 0 else avg + (1.0 - decay) * (p64 - avg)
        M = torch.maximum(p64.abs(), avg.abs()) if M is None else torch.maximum(M, torch.maximum(p64.abs(), avg.abs()))
    return avg, M


def test_trainer_averages_without_moving_the_training():
    built = _build(NAME)
    dev = built[6]
    plain, ema = _trainer(built), _trainer(built, avg="ema", avg_decay=0.9)
    assert plain.avg_mode is None and ema._avg_state is None and not ema.avg
    first = ema.averaged_state_dict()                           # before any update: the parameters themselves
    assert all(first[k] is ema.params[k] for k in ema.params)
    snaps = {k: [] for k in ema.params}
    for _ in range(3):
        l0, l1 = plain.step(dev), ema.step(dev)
        assert float(l0["loss"]) == float(l1["loss"])
        for k in snaps:
            snaps[k].append(ema.params[k].clone())
    assert plain._avg_state is None and not plain.avg
    assert set(ema.m) == set(plain.m) and set(ema.avg) == set(ema.m)
    for k in plain.params:
        assert torch.equal(plain.params[k], ema.params[k]), k
    for k in plain.m:
        assert torch.equal(plain.m[k], ema.m[k]) and torch.equal(plain.v[k], ema.v[k]), k
    s = ema.avg_state()
    assert s["n_averaged"] == 3 and s["updated"] == 1 and s["w"] == float(np.float32(1.0 - 0.9))
    worst, sd_avg = 0.0, ema.averaged_state_dict()
    assert set(sd_avg) == set(ema.params)
    for k in ema.avg:
        want, M = _ema64(snaps[k], 0.9)
        err, bound = (ema.avg[k].double() - want).abs(), 3 * 2.0 ** -23 * M
        nz = bound > 0
        assert bool((err[~nz] == 0).all()), k
        if bool(nz.any()):
            worst = max(worst, float((err[nz] / bound[nz]).max()))
        assert sd_avg[k] is ema.avg[k]
    print(f"trainer, ema 0.9, 3 steps: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst
    assert any(not torch.equal(ema.avg[k], ema.params[k]) for k in ema.avg)
    # the checkpoint form round-trips into a fresh trainer; another mode is refused
    asd = ema.averaging_state_dict()
    assert {k: asd[k] for k in ("mode", "decay", "warmup", "start", "every", "n_averaged")} == \
           {"mode": "ema", "decay": 0.9, "warmup": False, "start": 1, "every": 1, "n_averaged": 3}
    again = _trainer(built, avg="ema", avg_decay=0.9)
    again.load_averaging_state_dict(asd)
    assert again.avg_state()["n_averaged"] == 3 and all(torch.equal(again.avg[k], ema.avg[k]) for k in ema.avg)
    with pytest.raises(ValueError, match="mode"):
        _trainer(built, avg="swa").load_averaging_state_dict(asd)


def test_trainer_averages_once_per_accumulation_window_and_from_flush():
    built = _build(NAME)
    dev = built[6]
    tr = _trainer(built, avg="swa", accum_steps=2)
    for k in range(4):
        tr.step(dev)
    assert tr.adam_step == 2 and tr.num_it == 4 and tr.avg_state()["n_averaged"] == 2
    tr.step(dev)
    assert tr.avg_state()["n_averaged"] == 2                    # inside a window: no update, no average
    tr.flush()
    s = tr.avg_state()
    assert tr.adam_step == 3 and s["n_averaged"] == 3 and s["w"] == float(np.float32(1.0 / 3.0))


def test_frozen_parameters_are_their_own_average():
    built = _build(NAME)
    dev = built[6]
    tr = _trainer(built, avg="ema", avg_decay=0.9, freeze="lang")
    lang = [k for k in tr.params if k in tr.frozen]
    assert lang and len(lang) < len(tr.params)
    for _ in range(2):
        tr.step(dev)
    assert tr.avg_state()["n_averaged"] == 2
    # (the tensors the step covers: a parameter this model never reads gets no gradient, no m / v and no average either)
    assert not any(k in tr.avg for k in lang) and set(tr.avg) == set(tr.m) and tr.avg
    sd_avg = tr.averaged_state_dict()
    assert all(sd_avg[k] is tr.params[k] for k in lang) and all(sd_avg[k] is tr.avg[k] for k in tr.avg)
    # a parameter that becomes trainable joins the running average from its own value
    tr._freeze = None
    tr.set_param_groups(None)
    assert not tr.frozen and all(torch.equal(tr.avg[k], tr.params[k]) and tr.avg[k] is not tr.params[k] for k in lang)


def test_a_step_skipped_on_overflow_does_not_average():
    built = _build(NAME)
    dev = built[6]
    tr = _trainer(built, avg="ema", avg_decay=0.9, amp="f16", loss_scale=2.0 ** 40)
    before = {k: v.clone() for k, v in tr.params.items()}
    tr.step(dev)
    s, a = tr.scaler_state(), tr.avg_state()
    assert s["found_inf"] == 1 and s["adam_step"] == 0 and s["skipped"] == 1
    assert (a["n_averaged"], a["updated"], a["w"]) == (0, 0, 0.0)
    assert tr.avg and all(float(t.abs().max()) == 0.0 for t in tr.avg.values())         # never written
    sd_avg = tr.averaged_state_dict()
    assert all(sd_avg[k] is tr.params[k] and torch.equal(tr.params[k], before[k]) for k in tr.params)
    # the next, clean step (a scale the case does not overflow at) is the first update: a copy of the stepped parameters
    tr._write_opt_state(2.0 ** 10, 0, 0, 1)
    tr.step(dev)
    s, a = tr.scaler_state(), tr.avg_state()
    assert s["found_inf"] == 0 and s["adam_step"] == 1 and (a["n_averaged"], a["updated"], a["w"]) == (1, 1, 1.0)
    assert all(torch.equal(tr.avg[k], tr.params[k]) for k in tr.avg)
    assert any(not torch.equal(tr.params[k], before[k]) for k in tr.params)


# ---------------------------------------------------------------- 8: Learner
def _learner(tmp_path, uid, refresh, load_opt=False, resume_path="", **hip):
    torch.manual_seed(1234)                                     # (the Learner seeds its dropout masks from torch's seed)
    cfg, sd, batch, tg, c, mdl, dev, loss_fn = _build(NAME)
    sel_mod = importlib.import_module("vognet-pytorch_amd.mdl_selector")
    comm = comm_for(c)
    B, ncmp = batch["num_cmp_msk"].shape
    extra = {"ann_idx": np.arange(B, dtype=np.int64), "sent_idx": np.arange(B, dtype=np.int64),
             "permute": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64), "permute_inv": np.tile(np.arange(ncmp), (B, 1)).astype(np.int64)}
    one = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**batch, **tg, **extra}.items()}
    data = tu.DataWrap(path=tmp_path, train_dl=[one, one], valid_dl=[one], test_dl=[one])
    cfg.hip.weight_refresh = refresh
    for k, v in {"train_avg": "ema", "train_avg_decay": 0.9, "train_avg_eval": True, **hip}.items():
        cfg.hip[k] = v
    cfg.train.load_opt, cfg.train.resume_path = load_opt, str(resume_path)
    evl = sel_mod.get_mdl_loss_eval(cfg)["eval"](cfg, comm, torch.device("cuda", 0))
    learn = tu.Learner(uid=uid, data=data, mdl=mdl, loss_fn=loss_fn, cfg=cfg, eval_fn=evl, comm=comm)
    fwd = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}
    return learn, fwd


def _outputs(mdl, fwd):
    with torch.no_grad():
        out = mdl(fwd)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in OUT_KEYS}


@pytest.mark.parametrize("refresh", ["host", "device"])
def test_learner_validates_and_checkpoints_the_averaged_weights(tmp_path, refresh):
    learn, fwd = _learner(tmp_path, "A2", refresh)
    tr = learn.trainer
    assert tr.avg_mode == "ema" and tr.avg_decay == 0.9 and learn.avg_eval
    slot = None
    if refresh == "device":
        eng = learn.mdl.engine()
        slot = eng.make_slot(fwd, T=int(fwd["srl_arg_word_mask_len"].max()), graph=True)
        slot.launch()
        torch.cuda.synchronize()
        under_init = {k: slot.out[k].clone() for k in ("mdl_outs", "mdl_outs_eval")}
    learn.fit(epochs=2, lr=1e-4)                                # (ends with validate: the engine holds the averaged weights)
    assert tr.adam_step == 4 and tr.avg_state()["n_averaged"] == 4
    averaged = {k: v.clone() for k, v in tr.averaged_state_dict().items()}
    assert any(not torch.equal(averaged[k], tr.params[k]) for k in averaged)
    got = _outputs(learn.mdl, fwd)
    fresh = _build(NAME)[5]
    fresh.load_state_dict(averaged)
    want = _outputs(fresh, fwd)
    for k in OUT_KEYS:
        assert torch.equal(got[k], want[k]), k
    trained = _build(NAME)[5]
    trained.load_state_dict(tr.state_dict())
    assert not torch.equal(_outputs(trained, fwd)["mdl_outs"], want["mdl_outs"])         # not the trained weights'
    if slot is not None:                                        # captured before the first epoch: still valid, averaged weights
        out = slot.launch()
        torch.cuda.synchronize()
        slot.check()
        for k in ("mdl_outs", "mdl_outs_eval"):
            assert torch.equal(out[k], want[k]) and not torch.equal(out[k], under_init[k]), k
    learn.save_model_dict()
    ck = torch.load(learn.model_file.open("rb"), weights_only=False)
    asd = ck["averaging_state_dict"]
    assert set(asd) == {"mode", "decay", "warmup", "start", "every", "n_averaged", "averaged"}
    assert (asd["mode"], asd["decay"], asd["n_averaged"]) == ("ema", 0.9, 4)
    for k, v in tr.state_dict().items():                        # model_state_dict stays the TRAINED parameters
        assert torch.equal(ck["model_state_dict"][k], v.cpu()), k
    for k, v in tr.avg.items():
        assert torch.equal(asd["averaged"][k], v.cpu()), k
    from_ck = tu.averaged_weights_from_checkpoint(ck)
    assert all(torch.equal(from_ck[k], averaged[k].cpu()) for k in averaged)
    # 1 epoch + resume with the optimiser state + 1 epoch ends where the uninterrupted run did
    half, _ = _learner(tmp_path, "A1", refresh)
    half.fit(epochs=1, lr=1e-4)
    half.save_model_dict()
    rest, _ = _learner(tmp_path, "A1b", refresh, load_opt=True, resume_path=half.model_file)
    assert rest.trainer.avg_state()["n_averaged"] == 2 and rest.trainer.adam_step == 2 and rest.trainer.num_it == 2
    rest.fit(epochs=1, lr=1e-4)
    assert rest.trainer.avg_state()["n_averaged"] == 4 and set(rest.trainer.avg) == set(tr.avg)
    for k in tr.avg:
        assert torch.equal(rest.trainer.avg[k], tr.avg[k]), k
        assert torch.equal(rest.trainer.params[k], tr.params[k]), k


def test_only_val_refuses_a_checkpoint_without_averages(tmp_path):
    learn, _ = _learner(tmp_path, "N0", "host", train_avg="", train_avg_eval=False)
    assert learn.trainer.avg_mode is None and not learn.avg_eval
    learn.save_model_dict()
    ck = torch.load(learn.model_file.open("rb"), weights_only=False)
    assert "averaging_state_dict" not in ck
    main_mod = importlib.import_module("vognet-pytorch_amd.main_dist")
    with pytest.raises(ValueError, match="averaging_state_dict"):
        main_mod.main_dist("N0", **{"only_val": "True", "hip.train_avg": "ema", "hip.train_avg_eval": "True",
                                    "train.resume_path": str(learn.model_file), "misc.tmp_path": str(tmp_path)})


# ---------------------------------------------------------------- 9: two ranks
def _avg_worker(rank, world, port, name, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, sd, c, comm, sel, synth = _setup(name)
    tr = trn.FP32Trainer(cfg, comm, {k: torch.from_numpy(v) for k, v in sd.items()}, sel["loss"](cfg, comm), lr=1e-4,
                         avg="ema", avg_decay=0.9, clip_norm=1.0)
    dev = _rank_batch(synth, cfg, c, comm, rank, 2)
    for _ in range(2):
        tr.step(dev)
    torch.cuda.synchronize()
    stepped = (tr.avg_state(), {k: v.cpu().numpy() for k, v in tr.avg.items()})
    # what DistributedDataParallel's construction does after a resume: rank 1 loses its averages and gets rank 0's back
    if rank == 1:
        tr._write_avg_state(0)
        for v in tr.avg.values():
            v.zero_()
    try:
        tr.broadcast_from_rank0(with_optimizer=True)
        torch.cuda.synchronize()
        restored = bool(tr.avg_state()["n_averaged"] == 2 and set(tr.avg) == set(stepped[1])
                        and all(np.array_equal(tr.avg[k].cpu().numpy(), stepped[1][k]) for k in tr.avg))
    except Exception as e:                                      # (reported by the parent: a raise here would leave it waiting)
        restored = repr(e)
    q.put((rank, stepped[0], stepped[1], {k: v.cpu().numpy() for k, v in tr.params.items()}, restored))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_averages():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_avg_worker, args=(r, world, port, NAME, q)) for r in range(world)]
    for p in ps:
        p.start()
    got = {}
    for _ in range(world):
        r, st, avg, params, restored = q.get(timeout=300)
        got[r] = (st, avg, params, restored)
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert got[0][0] == got[1][0] and got[0][0]["n_averaged"] == 2
    assert set(got[0][1]) == set(got[1][1]) and len(got[0][1]) > 0
    for k in got[0][1]:
        assert np.array_equal(got[0][1][k].view(np.int32), got[1][1][k].view(np.int32)), k
    assert any(not np.array_equal(got[0][1][k], got[0][2][k]) for k in got[0][1])      # an average, not the parameters
    assert got[0][3] is True and got[1][3] is True, (got[0][3], got[1][3])             # broadcast_from_rank0 restored rank 1's
