"""CPU tests of the FiLM kink accounting of the oracle (`film_stack_forward(record=, gates=)`, handed through by
`spline_coupling_forward`): imposed leaky-ReLU decisions equal to the oracle's own change nothing, bit for bit; one flipped
decision on an element next to the kink moves the output by at most 0.99 |pre| and moves the gradient."""
import numpy as np
import torch

from conftest import sub
from oracle import radmmm_oracle as O


def _layer(golden):
    g = golden("spline_tiny.npz")
    shapes = {k: tuple(int(i) for i in v) for k, v in sub(g, "sp.shape.").items()}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in O.procedural_decoder_state(shapes, end_scale=0.05).items()}
    lens = torch.from_numpy(g["sp.in.lens"])
    mask = O.lengths_to_mask(lens)[:, None].float()
    return g, sd, mask


def _run(g, sd, mask, gates=None, record=None):
    p = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
    z = torch.from_numpy(g["sp.in.z"]).requires_grad_(True)
    ctx = torch.from_numpy(g["sp.in.ctx"]).requires_grad_(True)
    zo, log_s = O.spline_coupling_forward(p, "", z, ctx, mask, 2, use_bn=True, training=True, record=record, gates=gates)
    (0.5 * ((zo * mask) ** 2).sum() - (log_s * mask).sum()).backward()
    grads = {"z": z.grad, "ctx": ctx.grad, **{n: v.grad for n, v in p.items() if v.grad is not None}}
    return zo.detach(), log_s.detach(), grads


def test_own_decisions_as_gates_are_bit_identical(golden):
    g, sd, mask = _layer(golden)
    rec = {"ulps": 8, "pre": {}}
    zo, ls, gr = _run(g, sd, mask, record=rec)
    assert sorted(rec["pre"]) == [(0, "t"), (0, "x1"), (1, "t"), (1, "x1")]
    assert rec["leaky_total"] == 4 * 512 * int(mask.sum())
    zo0, ls0, gr0 = _run(g, sd, mask)                                   # no record, no gates: the path every other test takes
    assert torch.equal(zo, zo0) and torch.equal(ls, ls0) and all(torch.equal(gr[n], gr0[n]) for n in gr0)
    gates = {k: v > 0 for k, v in rec["pre"].items()}
    zo1, ls1, gr1 = _run(g, sd, mask, gates=gates)
    assert torch.equal(zo1, zo0) and torch.equal(ls1, ls0)
    assert gr1.keys() == gr0.keys() and len(gr0) > 20
    for n in gr0:
        assert torch.equal(gr1[n], gr0[n]), n


def test_one_flipped_gate_next_to_the_kink():
    """FiLM stack alone (its output is linear in the last block's activation): the valid element with the smallest |t| of the
    last block gets the other decision.  leaky(t) changes from t to 0.01 t or back, i.e. by 0.99 |t|; through
    0.5 * (. + x1r) and the `end` conv the output moves by at most 0.5 * 0.99 |t| * max |end.weight| -- and the gradient of
    that element's FiLM scale and bias (the cond conv's bias) sees the slope change by a factor of 100."""
    B, T, n_in, D, H, n_out, L = 2, 19, 4, 6, 16, 10, 2
    shapes = {"end.weight": (n_out, H, 1), "end.bias": (n_out,)}
    for j in range(L):
        for nm, co, ci, k in (("input_conv", H, n_in if j == 0 else H, 1), ("cond_conv", 2 * H, D, 1), ("hidden_conv", H, H, 5)):
            b = f"in_layers.{j}.{nm}.conv."
            shapes.update({b + "bias": (co,), b + "weight_g": (co, 1, 1), b + "weight_v": (co, ci, k)})
        b = f"in_layers.{j}.bn."
        shapes.update({b + "weight": (H,), b + "bias": (H,), b + "running_mean": (H,), b + "running_var": (H,)})
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in O.procedural_decoder_state(shapes, end_scale=0.05).items()}
    gen = torch.Generator().manual_seed(11)
    x, ctx = torch.randn(B, n_in, T, generator=gen), torch.randn(B, D, T, generator=gen)
    cot = torch.randn(B, n_out, T, generator=gen)
    mask = O.lengths_to_mask(torch.tensor([T, 12]))[:, None].float()

    def run(gates=None, record=None):
        p = {k: v.clone().requires_grad_("running" not in k) for k, v in sd.items()}
        q = O.film_stack_forward(p, "", x, ctx, mask, L, True, True, record, gates)
        (q * cot * mask).sum().backward()
        return q.detach(), {n: v.grad for n, v in p.items() if v.grad is not None}
    rec = {"pre": {}}
    q0, g0 = run(record=rec)
    gates = {k: v > 0 for k, v in rec["pre"].items()}
    key = (L - 1, "t")
    pre = rec["pre"][key]
    a = torch.where(mask.expand_as(pre) > 0, pre.abs(), torch.full_like(pre, float("inf")))
    idx = np.unravel_index(int(a.argmin()), a.shape)
    tiny = float(pre[idx].abs())
    assert 0 < tiny < 1e-2 * float(pre.abs().max())
    gates[key] = gates[key].clone()
    gates[key][idx] = ~gates[key][idx]
    q1, g1 = run(gates=gates)
    dq = (q1 - q0).abs()
    wmax = float(sd["end.weight"].abs().max())
    assert 0 < float(dq.max()) <= 0.5 * 0.99 * tiny * wmax * (1 + 1e-5)
    moved = torch.zeros_like(dq, dtype=torch.bool)
    moved[idx[0], :, idx[2]] = True                               # a 1x1 conv: only that frame of that item
    assert float(dq[~moved].max()) == 0.0
    n = f"in_layers.{L - 1}.cond_conv.conv.bias"
    assert not torch.equal(g1[n], g0[n])
    assert float((g1[n] - g0[n]).abs().max()) > 1e-3 * float(g0[n].abs().max())
