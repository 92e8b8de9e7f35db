"""Torch restatements for the factored Q / K / V projections of mul_tx's layer 0 (`vog_attn_vl`, include/vog_hip.h), shared by
tests/test_train_qkv_host.py (float64, no GPU) and tests/test_gpu_train_qkv.py: the cases, the dense reference (autograd through
the attention on the concatenated tokens) and the factored form written out - forward and backward - with an optional rounding
of the operands of every product it issues."""
import functools
import math

import torch

# (n_q, nc_v, nfrm, n, nsrl, dobj, dlang, lang_per_vid, H, rel): the smallest shapes at which each piece can go wrong
SHAPES = [
    (1, 1, 1, 1, 1, 5, 3, 0, 2, True),            # one token
    (2, 2, 2, 7, 3, 32, 16, 0, 3, True),          # argument rows shared by the videos of a query, the small goldens' widths
    (2, 2, 2, 7, 3, 32, 16, 1, 3, True),          # argument rows per video
    (2, 1, 3, 5, 5, 33, 15, 0, 3, True),          # odd column split: no aligned 16-byte access into a weight's column block
    (1, 3, 2, 9, 2, 13, 7, 1, 4, False),          # no bias, uneven heads
    (2, 1, 2, 20, 5, 512, 256, 0, 3, True),       # the workload's own row: N = 100, d = 768, head 256
    (1, 1, 3, 100, 2, 64, 32, 0, 3, True),        # 300 token rows per language row, N = 200 over several 64-row tiles
    (3, 1, 33, 2, 3, 24, 8, 0, 2, True),          # 33 sequences per group: the second reduce stage
    (2, 1, 2, 3, 9, 5, 2, 0, 2, True),            # d = 7: the scalar kernels; 9 arguments: two argument chunks of the reduce
]
VW, VH = 720.0, 405.0


def dims(shape):
    n_q, nc_v, nfrm, n, nsrl, dobj, dlang, lpv, H, rel = shape
    S, G = n_q * nc_v * nfrm, n_q * (nc_v if lpv else 1)
    return dict(S=S, G=G, spg=S // G, N=nsrl * n, d=dobj + dlang, n=n, nsrl=nsrl, dobj=dobj, dlang=dlang, H=H, rel=rel, nfrm=nfrm)


def conc(ps, mlang, D):
    """[S, N, d] tokens (s, arg, p) = [ps[(s, p)] | mlang[(g(s), arg)]] (vog_conc_f32_fwd with the mask already applied)."""
    S, n, nsrl = D["S"], D["n"], D["nsrl"]
    vis = ps.reshape(S, 1, n, D["dobj"]).expand(S, nsrl, n, D["dobj"])
    lg = mlang.reshape(D["G"], 1, nsrl, D["dlang"]).expand(D["G"], D["spg"], nsrl, D["dlang"]).reshape(S, nsrl, 1, D["dlang"])
    return torch.cat([vis, lg.expand(S, nsrl, n, D["dlang"])], -1).reshape(S, D["N"], D["d"])


@functools.lru_cache(maxsize=None)
def case(shape, masked):
    """fp32 inputs of one geometry (read-only). masked: a random 0 / 1 mask whose first query is fully masked; else no mask."""
    D = dims(shape)
    g = torch.Generator().manual_seed(sum((i + 3) * v for i, v in enumerate(shape[:8])))
    S, n, d, H = D["S"], D["n"], D["d"], D["H"]
    c = dict(D, shape=shape)
    c["ps"] = torch.randn(S * n, D["dobj"], generator=g)
    c["lang"] = torch.randn(D["G"] * D["nsrl"], D["dlang"], generator=g)
    c["ws"] = [torch.randn(d, d, generator=g) / math.sqrt(d) for _ in range(3)]
    c["props"] = torch.rand(S * n, 7, generator=g) * torch.tensor([VW, VH, VW, VH, float(D["nfrm"]), 1., 1.])
    c["pe_w"], c["pe_b"] = torch.randn(H, 5, generator=g), torch.randn(H, generator=g) * 0.3
    c["d_cat"] = torch.randn(S, D["N"], d, generator=g)
    c["bx"] = (c["props"][:, :5] / torch.tensor([VW, VH, VW, VH, float(D["nfrm"])])).reshape(S, n, 5) if D["rel"] else None
    c["msk"] = None
    if masked:
        m = (torch.rand(D["G"], D["nsrl"], generator=g) < 0.6).to(torch.int64)
        m[:D["G"] // shape[0]] = 0                                     # the argument rows of query 0
        c["msk"] = m.reshape(-1)
    return c


def core(q, k, v, bx, pe_w, pe_b, H, nsrl, mm=torch.matmul):
    """Concatenated heads softmax((Q K^T + bias) / sqrt(d)) V from q, k, v [S, N, d] (transformer_code.py:136-162); mm = the
    product of the three matrix products."""
    d = q.shape[-1]
    c = -(-d // H)
    outs, off = [], 0
    for h in range(H):
        dh = min(c, d - off)
        lg = mm(q[..., off:off + dh], k[..., off:off + dh].transpose(1, 2))
        if bx is not None:
            diff = bx.unsqueeze(2) - bx.unsqueeze(1)
            lg = lg + torch.relu(diff @ pe_w[h] + pe_b[h]).repeat(1, nsrl, nsrl)
        outs.append(mm(torch.softmax(lg / math.sqrt(d), dim=-1), v[..., off:off + dh]))
        off += dh
    return torch.cat(outs, -1)


def _mask_col(c, dt):
    return torch.ones(c["G"] * c["nsrl"], 1, dtype=dt) if c["msk"] is None else c["msk"].to(dt).reshape(-1, 1)


def dense(c, dt=torch.float32, attn=None):
    """Autograd through the dense operator on the concatenated tokens -> cat, g_wq / g_wk / g_wv, g_pe_w / g_pe_b, d_ps, d_lang.
    attn(x, wq, wk, wv, bx, pe_w, pe_b, H, nsrl): the dense attention (default: projections by plain matmul, then `core`)."""
    lv = {k: c[k].to(dt).clone().requires_grad_(True) for k in ("ps", "lang", "pe_w", "pe_b")}
    ws = [w.to(dt).clone().requires_grad_(True) for w in c["ws"]]
    bx = c["bx"].to(dt) if c["bx"] is not None else None
    x = conc(lv["ps"], lv["lang"] * _mask_col(c, dt), c)
    if attn is None:
        cat = core(x @ ws[0].t(), x @ ws[1].t(), x @ ws[2].t(), bx, lv["pe_w"], lv["pe_b"], c["H"], c["nsrl"])
    else:
        cat = attn(x, ws[0], ws[1], ws[2], bx, lv["pe_w"], lv["pe_b"], c["H"], c["nsrl"])
    (cat * c["d_cat"].to(dt)).sum().backward()
    rel = c["rel"]
    return dict(cat=cat.detach(), g_wq=ws[0].grad, g_wk=ws[1].grad, g_wv=ws[2].grad, g_pe_w=lv["pe_w"].grad if rel else None,
                g_pe_b=lv["pe_b"].grad if rel else None, d_ps=lv["ps"].grad, d_lang=lv["lang"].grad)


def factored(c, dt=torch.float32, P=torch.matmul, mm=torch.matmul):
    """The factored operator written out, forward and backward (autograd only through `core`, from q, k, v to dq, dk, dv).
    P(a, b): the product of the projections and gradient products - plain, or with both operands rounded to a 16-bit type, which
    rounds exactly what the device rounds: ps, mask * lang, the weights' column blocks, the summed dPv / dPl. mm: `core`'s."""
    S, G, spg, n, nsrl, d, dobj = c["S"], c["G"], c["spg"], c["n"], c["nsrl"], c["d"], c["dobj"]
    ps, mk = c["ps"].to(dt), _mask_col(c, dt)
    ml = c["lang"].to(dt) * mk
    ws = [w.to(dt) for w in c["ws"]]
    bx = c["bx"].to(dt) if c["bx"] is not None else None
    pe_w, pe_b = (c[k].to(dt).clone().requires_grad_(True) for k in ("pe_w", "pe_b"))
    qkv = []
    for w in ws:
        pv, pl = P(ps, w[:, :dobj].t()), P(ml, w[:, dobj:].t())                  # [S*n, d], [G*nsrl, d]
        t = pv.reshape(S, 1, n, d) + pl.reshape(G, 1, nsrl, 1, d).expand(G, spg, nsrl, 1, d).reshape(S, nsrl, 1, d)
        qkv.append(t.reshape(S, nsrl * n, d).clone().requires_grad_(True))
    cat = core(qkv[0], qkv[1], qkv[2], bx, pe_w, pe_b, c["H"], nsrl, mm)
    (cat * c["d_cat"].to(dt)).sum().backward()
    out = dict(cat=cat.detach(), g_pe_w=pe_w.grad if c["rel"] else None, g_pe_b=pe_b.grad if c["rel"] else None)
    d_ps, d_lang = torch.zeros_like(ps), torch.zeros_like(ml)
    for name, w, t in zip(("g_wq", "g_wk", "g_wv"), ws, qkv):
        dT = t.grad.reshape(S, nsrl, n, d)
        dpv = dT.sum(1).reshape(S * n, d)                                          # over the arguments
        dpl = dT.sum(2).reshape(G, spg, nsrl, d).sum(1).reshape(G * nsrl, d) * mk   # over the proposals, then the group's sequences
        out[name] = torch.cat([P(dpv.t(), ps), P(dpl.t(), ml)], 1)
        d_ps = d_ps + P(dpv, w[:, :dobj])
        d_lang = d_lang + P(dpl, w[:, dobj:])
    out["d_ps"], out["d_lang"] = d_ps, d_lang * mk
    return out
