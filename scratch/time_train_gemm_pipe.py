"""The pipelined 16-bit tile GEMM (`gemm_amp="pipe"`: gemm16_pipe_kernel, csrc/train_gemm.hip) against the 128 x 64 tile kernel
(`gemm16_kernel<T, false>`), timed alternately in one process, amp bf16:

  (a) the operator alone, event-timed, at every distinct vector product the cfg-2 and cfg-5 amp steps issue. The list below was
      taken once by logging gemm_f32_b's arguments over one step of each configuration. Every product of the step belongs to a
      linear layer (M rows, N outputs, K inputs) and has one of three layouts, which `vog_linear_f32` issues as
          y   [M, N, K]  A row-major, B k-contiguous        (forward only call)
          g_w [N, K, M]  A column-major, B row-major        (call with the weight gradient only, minus the forward only call)
          d_x [M, K, N]  A row-major, B row-major           (call with the input gradient only, minus the forward only call)
      so a layer (M, N, K) is timed in those three calls; the two backward calls also run the row kernel that writes dpre, the
      same in both arms. Batched products: `vog_attn_f32` forward + backward at cfg 2's mul_tx geometry (the per-head products
      100 x 100 x 256 over 40 sequences; the heads of obj_tx and of cfg 5 split 171 / 170 or have 25 tokens and stay scalar).
      Median of `--rounds` rounds of `--calls` calls and their spread (max - min) per figure;
  (b) the cfg-2 and cfg-5 training steps in amp bf16 with lstm_amp="split" in every arm: the parent commit's package
      (`--parent DIR`: a built checkout of it), this tree's default, and gemm_amp="pipe" - and, before anything is timed, the amp
      and the fp32 parameters after 3 steps of parent and default compared bit for bit, and pipe's against the default's.

`--trace-steps N` instead runs N cfg-2 amp bf16 steps with gemm_amp="pipe" and nothing else, for a kernel trace taken from outside.

    python scratch/time_train_gemm_pipe.py OUT.json [--rounds N] [--calls N] [--steps K] [--parent DIR] [--operator-only]
"""
import importlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests.gpu_util import comm_for  # noqa: E402
from time_finetune import load_parent, stats, timed  # noqa: E402
from time_train_lstm import CFG2, CFG5, _setup  # noqa: E402

trn = importlib.import_module("vognet-pytorch_amd.train")
BW = importlib.import_module("vognet-pytorch_amd.backward")
L = importlib.import_module("vognet-pytorch_amd.lib")

# (M, N, K) of the layers behind the vector products of one amp step, and how often each layout occurs in a cfg-2 step (y, g_w, d_x);
# cfg 5 has the same mul_tx / obj_tx rows and the language rows at M = 192 / 80 in place of 48 / 20
LAYERS = [
    ("mul_tx q/k/v/o", 4000, 768, 768, (8, 4, 4)), ("mul_tx ffn1", 4000, 384, 768, (2, 1, 1)), ("mul_tx ffn2", 4000, 768, 384, (2, 1, 1)),
    ("mul_tx head", 4000, 256, 768, (2, 1, 1)),
    ("obj_tx q/k/v/o", 800, 512, 512, (8, 4, 4)), ("obj_tx ffn1", 800, 256, 512, (2, 1, 1)), ("obj_tx ffn2", 800, 512, 256, (2, 1, 1)),
    ("visual encoder", 800, 256, 2048, (2, 1, 0)), ("language out", 160, 256, 3072, (2, 1, 0)),
    ("lstm input l0", 48, 4096, 512, (2, 2, 2)), ("lstm input l1", 48, 4096, 2048, (2, 2, 2)), ("lstm recurrent dW", 48, 4096, 1024, (0, 4, 0)),
    ("lstm out proj", 48, 256, 2048, (1, 1, 1)), ("verb", 20, 256, 512, (1, 1, 1)),
    ("cfg5 lstm input l0", 192, 4096, 512, (2, 2, 2)), ("cfg5 lstm input l1", 192, 4096, 2048, (2, 2, 2)),
    ("cfg5 lstm recurrent dW", 192, 4096, 1024, (0, 4, 0)), ("cfg5 lstm out proj", 192, 256, 2048, (1, 1, 1)), ("cfg5 verb", 80, 256, 512, (1, 1, 1)),
]
ATTN = ("mul_tx attention cfg2", 40, 100, 20, 768, 3)          # S, N, n, d, H
FORMS = ("tile", "pipe")


def _alternate(fns, calls, rounds):
    """fns: {(form, what): callable}; the forms alternate inside every round; round 0 warms up -> {key: stats} in ms per call"""
    lib = L.load()
    ms = {k: [] for k in fns}
    try:
        lib.vog_train_set_int(b"amp", 1)
        for r in range(rounds + 1):
            for (form, what), fn in fns.items():
                lib.vog_train_set_int(b"gemm_amp_pipe", int(form == "pipe"))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r:
                    ms[(form, what)].append(e0.elapsed_time(e1) / calls)
    finally:
        lib.vog_train_set_int(b"gemm_amp_pipe", 0)
        lib.vog_train_set_int(b"amp", 0)
    return {k: stats(v) for k, v in ms.items()}


def _verdict(row, what):
    t, p = row[f"tile_{what}"], row[f"pipe_{what}"]
    return {"tile_minus_pipe_ms": t["median"] - p["median"], "pipe_over_tile": p["median"] / t["median"],
            "beyond_spread": bool(abs(t["median"] - p["median"]) > max(t["spread"], p["spread"]))}


def operator_alone(calls, rounds):
    lib = L.load()
    out = {}
    for name, M, N, K, count in LAYERS:
        g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
        x, w = torch.randn(M, K, generator=g).cuda(), (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda()
        b, dy = (torch.randn(N, generator=g) * 0.1).cuda(), torch.randn(M, N, generator=g).cuda()
        scr = torch.empty(int(lib.vog_linear_f32_scratch_bytes(M, N)), dtype=torch.uint8, device="cuda")
        calls_of = {"fwd": lambda: BW.linear_f32(x, w, b, True, scratch=scr),
                    "fwd_gw": lambda: BW.linear_f32(x, w, b, True, dy=dy, want_w=True, want_b=False, want_dx=False, scratch=scr),
                    "fwd_dx": lambda: BW.linear_f32(x, w, b, True, dy=dy, want_w=False, want_b=False, want_dx=True, scratch=scr)}
        res = _alternate({(form, what): fn for what, fn in calls_of.items() for form in FORMS}, calls, rounds)
        row = {"M": M, "N": N, "K": K, "products_per_cfg2_step_y_gw_dx": count, "calls_per_timing": calls,
               **{f"{form}_{what}": v for (form, what), v in res.items()}}
        for what in calls_of:
            row[what] = _verdict(row, what)
        # the backward product alone: the call minus the forward only call (medians)
        for what, prod in (("fwd_gw", "g_w"), ("fwd_dx", "d_x")):
            row[prod + "_alone_ms"] = {form: row[f"{form}_{what}"]["median"] - row[f"{form}_fwd"]["median"] for form in FORMS}
        out[f"{name} ({M}, {N}, {K})"] = row
        print("linear", name, (M, N, K), json.dumps({f"{f}_{w}": round(row[f"{f}_{w}"]["median"] * 1e3, 1) for w in calls_of for f in FORMS}), flush=True)
        del scr
    name, S, N, n, d, H = ATTN
    g = torch.Generator().manual_seed(S * 1000 + N)
    x, d_cat = torch.randn(S * N, d, generator=g).cuda(), torch.randn(S * N, d, generator=g).cuda()
    w = {k: (torch.randn(d, d, generator=g) / math.sqrt(d)).cuda() for k in ("wq", "wk", "wv")}
    props = (torch.rand(S * n, 7, generator=g) * torch.tensor([720., 405., 720., 405., 10., 1., 1.])).cuda()
    pe = (torch.randn(H, 5, generator=g).cuda(), (torch.randn(H, generator=g) * 0.3).cuda())
    boxes = BW._Boxes(props, 720.0, 405.0, 10.0)
    scr = torch.empty(int(lib.vog_attn_f32_scratch_bytes(S, N, n, d)), dtype=torch.uint8, device="cuda")
    res = _alternate({(form, "fwd_bwd"): (lambda: BW._attn_call(w, pe, x, S, N, n, H, boxes, d_cat=d_cat, scratch=scr)) for form in FORMS},
                     calls, rounds)
    row = {"S": S, "N": N, "n": n, "d": d, "H": H, "calls_per_timing": calls, **{f"{form}_{what}": v for (form, what), v in res.items()}}
    row["fwd_bwd"] = _verdict(row, "fwd_bwd")
    out[name] = row
    print("attn", json.dumps({f: round(row[f"{f}_fwd_bwd"]["median"] * 1e3, 1) for f in FORMS}), flush=True)
    return out


def _bit_equal(mk_a, mk_b, dev):
    a, b = mk_a(), mk_b()
    for _ in range(3):
        a.step(dev)
        b.step(dev)
    torch.cuda.synchronize()
    return bool(set(a.params) == set(b.params) and all(torch.equal(a.params[k], b.params[k]) for k in b.params))


def step(name, rounds, steps, parent):
    cfg, c, sdt, dev, loss_fn = _setup(name)

    def mk(amp, **kw):
        return trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp=amp, **kw)

    summary = {"case": name, "amp": "bf16", "lstm_amp": "split", "rounds": rounds, "steps_per_round": steps, "parent_timed": parent is not None}
    fns = {}
    if parent is not None:
        ptrn, psel = parent
        ploss = psel.get_mdl_loss_eval(cfg)["loss"](cfg, comm_for(c))

        def mk_parent(amp, **kw):
            return ptrn.FP32Trainer(cfg, comm_for(c), sdt, ploss, lr=1e-4, amp=amp, **kw)
        summary["amp_params_bit_equal_to_parent_after_3_steps"] = _bit_equal(lambda: mk_parent("bf16", lstm_amp="split"),
                                                                             lambda: mk("bf16", lstm_amp="split"), dev)
        summary["fp32_params_bit_equal_to_parent_after_3_steps"] = _bit_equal(lambda: mk_parent(None), lambda: mk(None), dev)
        assert summary["amp_params_bit_equal_to_parent_after_3_steps"] and summary["fp32_params_bit_equal_to_parent_after_3_steps"], summary
        fns["parent"] = lambda t=mk_parent("bf16", lstm_amp="split"): t.step(dev)
    summary["pipe_params_bit_equal_to_default_after_3_steps"] = _bit_equal(lambda: mk("bf16", lstm_amp="split"),
                                                                           lambda: mk("bf16", lstm_amp="split", gemm_amp="pipe"), dev)
    assert summary["pipe_params_bit_equal_to_default_after_3_steps"], "gemm_amp='pipe' changed the bits of the amp step"
    fns["default"] = lambda t=mk("bf16", lstm_amp="split"): t.step(dev)
    fns["pipe"] = lambda t=mk("bf16", lstm_amp="split", gemm_amp="pipe"): t.step(dev)
    res = {m: [] for m in fns}
    for _ in range(rounds):                                         # the arms alternate: drift hits them all alike
        for m, fn in fns.items():
            res[m].append(timed(fn, steps))
    arms = {m: stats(v) for m, v in res.items()}
    if parent is not None:
        p, dflt = arms["parent"], arms["default"]
        dflt["minus_parent_median_ms"] = dflt["median"] - p["median"]
        dflt["within_parent_spread"] = bool(abs(dflt["median"] - p["median"]) <= p["spread"])
    arms["pipe"]["minus_default_median_ms"] = arms["pipe"]["median"] - arms["default"]["median"]
    arms["pipe"]["beyond_spread"] = bool(abs(arms["pipe"]["minus_default_median_ms"]) > max(arms["pipe"]["spread"], arms["default"]["spread"]))
    summary["arms_ms"] = arms
    lib, n = L.load(), __import__("ctypes").c_int(-1)
    lib.vog_train_set_int(b"gemm_amp_pipe_launches", 0)
    fns["pipe"]()
    lib.vog_train_get_int(b"gemm_amp_pipe_launches", __import__("ctypes").byref(n))
    summary["pipe_launches_per_step"] = n.value
    print(name, json.dumps({m: [round(v["median"], 3), round(v["spread"], 3)] for m, v in arms.items()}), flush=True)
    return summary


def main():
    out = sys.argv[1]
    arg = lambda flag, dflt: int(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else dflt
    torch.cuda.set_device(0)
    if "--trace-steps" in sys.argv:
        cfg, c, sdt, dev, loss_fn = _setup(CFG2)
        t = trn.FP32Trainer(cfg, comm_for(c), sdt, loss_fn, lr=1e-4, amp="bf16", lstm_amp="split", gemm_amp="pipe")
        for _ in range(arg("--trace-steps", 10)):
            t.step(dev)
        torch.cuda.synchronize()
        return
    rounds, calls, steps = arg("--rounds", 5), arg("--calls", 10), arg("--steps", 10)
    parent = load_parent(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    summary = {"device": torch.cuda.get_device_name(0), "rounds": rounds}
    summary["operator_alone_ms"] = operator_alone(calls, rounds)
    if "--operator-only" not in sys.argv:
        summary["cfg2_step"] = step(CFG2, rounds, steps, parent)
        summary["cfg5_step"] = step(CFG5, rounds, steps, parent)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
