"""numpy float64 restatement of torch.optim.Adam / torch.optim.AdamW (single-tensor form, amsgrad and maximize off), the
reference of the fused step's tests (rad_mmm_amd/csrc/optim.hip adam_kernel, rad_mmm_amd.optim.FlatAdam).

    adam_step(p, g, m, v, t, ...)      one update IN PLACE; t is the step count AFTER this step (1 for the first)
    run(p0, grads, ...)                a trajectory: the parameters after every step
    within_bar(got, want, steps)       the GPU tests' bar (tests/test_radam.py:55: rtol 2e-6, atol 2e-7 over several steps;
                                       its one-step form, rtol 1e-6, atol 1e-7, after a single step)

`flaw` plants one wrong variant, which the bar has to reject (tests/test_adam_cpu.py):
    "decay_swapped"   coupled and decoupled weight decay exchanged
    "eps_in_sqrt"     sqrt(v / (1 - b2^t) + eps) instead of sqrt(v) / sqrt(1 - b2^t) + eps
    "bias_t_minus_1"  the bias corrections from t - 1 (a counter read before it advanced)
    "count_skipped"   the counter advances on a skipped step (run(..., skip=))"""
import numpy as np

RTOL, ATOL = 2e-6, 2e-7
RTOL1, ATOL1 = 1e-6, 1e-7


def adam_step(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, clip=None,
              flaw=None):
    b1, b2 = betas
    g = np.asarray(g, dtype=np.float64)
    if clip is not None:
        g = g * clip
    if flaw == "decay_swapped":
        decoupled = not decoupled
    if decoupled:
        p *= 1.0 - lr * weight_decay
    elif weight_decay != 0.0:
        g = g + weight_decay * p
    m *= b1
    m += (1.0 - b1) * g
    v *= b2
    v += (1.0 - b2) * g * g
    tb = t - 1 if flaw == "bias_t_minus_1" else t
    bc1 = 1.0 - b1 ** tb if tb > 0 else 1.0 - b1           # (t - 1 = 0 would divide by zero: the planted flaw stays finite)
    bc2 = 1.0 - b2 ** tb if tb > 0 else 1.0 - b2
    if flaw == "eps_in_sqrt":
        denom = np.sqrt(v / bc2 + eps)
    else:
        denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p -= (lr / bc1) * m / denom


def run(p0, grads, skip=None, clips=None, flaw=None, **kw):
    """p0: array; grads: one array per step; skip: per step, True = the step is a no-op (and does not count).  Returns
    (list of the parameters after every step, m, v, t)."""
    p = np.array(p0, dtype=np.float64)
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    out = []
    for k, g in enumerate(grads):
        if skip is not None and skip[k]:
            if flaw == "count_skipped":
                t += 1
        else:
            t += 1
            adam_step(p, g, m, v, t, clip=None if clips is None else clips[k], flaw=flaw, **kw)
        out.append(p.copy())
    return out, m, v, t


def within_bar(got, want, steps):
    rtol, atol = (RTOL1, ATOL1) if steps == 1 else (RTOL, ATOL)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= atol + rtol * np.abs(want)))


def worst_over_bar(got, want, steps):
    rtol, atol = (RTOL1, ATOL1) if steps == 1 else (RTOL, ATOL)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))
