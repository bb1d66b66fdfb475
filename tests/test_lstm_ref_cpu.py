"""The float64 restatement of the LSTM recurrence (tests/_lstm_ref.py) that the GPU tests of csrc/lstm.hip are judged
against, pinned on the CPU: it equals torch.nn.LSTM on packed batches, defines len = 0, and reproduces the gradient
growth that the backward kernel's fp16 operand scale has to survive.  No GPU, no library."""
import pytest
import torch
from torch import nn

from _lstm_ref import bilstm_ref, bilstm_ref_grads, dwhh_from_dG, growth_case


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("B,T,I,H,lens", [(3, 7, 5, 4, None), (5, 11, 6, 9, [11, 3, 1, 7, 11]), (4, 9, 3, 17, [2, 9, 5, 1]),
                                          (2, 1, 3, 2, None), (3, 6, 4, 8, [4, 2, 5])])
def test_restatement_matches_nn_lstm_double(B, T, I, H, lens):
    g = torch.Generator().manual_seed(10 * B + H)
    lstm = nn.LSTM(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) - 0.5) * 1.2)
    x = torch.randn(B, T, I, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64)
    if lens is None:
        y_ref = lstm(x)[0]
    else:
        packed = nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False)
        y_ref = nn.utils.rnn.pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=T)[0]
    (y_ref * dy).sum().backward()
    want = {n: p.grad.clone() for n, p in lstm.named_parameters()}
    want["x"] = x.grad.clone()

    x2 = x.detach().clone().requires_grad_(True)
    P = {n: p.detach().clone().requires_grad_(True) for n, p in lstm.named_parameters()}
    Gs = [x2 @ P["weight_ih_l0" + sfx].t() + P["bias_ih_l0" + sfx] + P["bias_hh_l0" + sfx] for sfx in ("", "_reverse")]
    G = torch.stack(Gs, 2).view(B, T, 2, 4, H)
    G.retain_grad()
    W_hh = torch.stack((P["weight_hh_l0"], P["weight_hh_l0_reverse"]))
    y, c, gates = bilstm_ref(G, W_hh, lens)
    assert _rel(y.reshape(B, T, 2 * H), y_ref.detach()) < 1e-12
    (y.reshape(B, T, 2 * H) * dy).sum().backward()
    assert _rel(x2.grad, want["x"]) < 1e-12
    for n, p in P.items():
        assert _rel(p.grad, want[n]) < 1e-12, n
    # what the kernel's caller builds from dG is the same recurrent weight gradient
    dW = dwhh_from_dG(G.grad, y.detach())
    assert _rel(dW[0], want["weight_hh_l0"]) < 1e-12 and _rel(dW[1], want["weight_hh_l0_reverse"]) < 1e-12
    if lens is not None:
        for b, n in enumerate(lens):
            assert torch.all(y[b, n:] == 0) and torch.all(c[b, n:] == 0) and torch.all(gates[b, n:] == 0)
            assert torch.all(G.grad[b, n:] == 0)


def test_empty_item_is_zero_and_leaves_the_others_alone():
    g = torch.Generator().manual_seed(5)
    B, T, H = 4, 6, 5
    G = torch.randn(B, T, 2, 4, H, generator=g)
    W = torch.randn(2, 4 * H, H, generator=g) * 0.4
    dy = torch.randn(B, T, 2, H, generator=g)
    lens = [6, 0, 3, 1]
    r = bilstm_ref_grads(G, W, lens, dy)
    for k in ("y", "c", "gates", "dG"):
        assert torch.all(r[k][1] == 0), k
    keep = [0, 2, 3]
    q = bilstm_ref_grads(G[keep], W, [lens[i] for i in keep], dy[keep])
    for k in ("y", "c", "gates", "dG"):
        assert _rel(r[k][keep], q[k]) < 1e-13, k          # (the BLAS may block a batch of 3 and of 4 differently)
    assert _rel(r["dW"], q["dW"]) < 1e-14


def test_gradient_growth_premise():
    """max|dG| / max|dy| with a forget bias of 3 and same-sign upstream gradient: beyond the 1875 that a scale derived from
    max|dy| (64 / max|dy|, clamp at 60000) can leave for H = 64, T = 400; harmless for H = 16, T = 800."""
    big = bilstm_ref_grads(*growth_case(64, 400)[:2], None, growth_case(64, 400)[2])
    ratio_big = float(big["dG"].abs().max())
    small = bilstm_ref_grads(*growth_case(16, 800)[:2], None, growth_case(16, 800)[2])
    ratio_small = float(small["dG"].abs().max())
    print(f"growth: H=64 T=400 max|dG|/max|dy| = {ratio_big:.3g}; H=16 T=800: {ratio_small:.3g}")
    assert ratio_big > 1875
    assert ratio_small < 100
