"""Float64 restatement of torch.optim.Adam with parameter groups and L2 weight decay, shared by tests/test_finetune_host.py
(which pins it against torch.optim.Adam itself) and tests/test_gpu_finetune.py (which compares the kernels with it)."""
import math


def adam64_groups(p, g, m, v, step, spans, b1, b2, eps, coef=1.0):
    """One step over lists of float64 tensors. spans: [(first, count, lr, weight_decay)] over the lists' positions; tensors no
    span covers come back unchanged. The gradient that enters the moments is g * coef + weight_decay * p (coef: the clip /
    unscale factor; the decay is not clipped). -> (p, m, v, terms), terms = the sum of the magnitudes added into m per element
    (what its rounding error is relative to), None for uncovered tensors."""
    p, m, v = list(p), list(m), list(v)
    terms = [None] * len(p)
    for first, count, lr, wd in spans:
        for i in range(first, first + count):
            gi = g[i].double() * coef + wd * p[i]
            terms[i] = (b1 * m[i]).abs() + ((1 - b1) * g[i].double() * coef).abs() + ((1 - b1) * wd * p[i]).abs()
            m[i] = b1 * m[i] + (1 - b1) * gi
            v[i] = b2 * v[i] + (1 - b2) * gi * gi
            denom = v[i].sqrt() / math.sqrt(1 - b2 ** step) + eps
            p[i] = p[i] - lr / (1 - b1 ** step) * (m[i] / denom)
    return p, m, v, terms
