"""Plain restatement of the bidirectional LSTM recurrence of csrc/lstm.hip in torch on the CPU (float64 by default), taking
what the kernels take rather than what nn.LSTM takes:

    G     [B, T, 2, 4, H]  pre-activations x W_ih^T + b per direction and gate (order i, f, g, o)
    W_hh  [2, 4H, H]
    lens  [B] ints or None (all T frames valid)

Packed-sequence semantics as the kernel header states them: frames t >= len give h = c = 0 and all-zero saved gates, the
reverse direction thereby starts at each item's own last frame.  len = 0 is allowed (torch's packing refuses it): an
all-zero item with zero gradient.  Gradients come from autograd on the same graph.  No test functions in here."""
import os

import torch


def bilstm_ref(G, W_hh, lens=None, dtype=torch.float64, noise=0.0):
    """-> y, c [B, T, 2, H], gates [B, T, 2, 4, H] in `dtype`.  G / W_hh may require grad (then they must already be `dtype`).
    noise > 0 models inexact recurrent products the way a split-f16 product is inexact -- relative to the sum of the
    magnitudes of its terms: a += noise * xi * (|h| |W_hh|^T), xi uniform in +-1 (seeded).  It measures how far a case's own
    dynamics carry such an error (its conditioning) without looking at any kernel."""
    B, T, _, _, H = G.shape
    G = G.to(dtype)
    Wt = W_hh.to(dtype).view(2, 4 * H, H).transpose(1, 2)                    # [2, H, 4H]
    ln = torch.full((B,), T, dtype=torch.long) if lens is None else torch.as_tensor(lens, dtype=torch.long)
    gen = torch.Generator().manual_seed(0)
    h = torch.zeros(2, B, H, dtype=dtype)
    c = torch.zeros(2, B, H, dtype=dtype)
    ys, cs, gs = [[None] * T, [None] * T], [[None] * T, [None] * T], [[None] * T, [None] * T]
    zero = torch.zeros((), dtype=dtype)
    for s in range(T):
        tt = (s, T - 1 - s)
        a = torch.bmm(h, Wt)                                                 # [2, B, 4H]
        if noise:
            xi = 2 * torch.rand(a.shape, generator=gen, dtype=torch.float64) - 1
            a = a + (noise * xi * torch.bmm(h.detach().abs().double(), Wt.detach().abs().double())).to(dtype)
        pre = a.view(2, B, 4, H) + torch.stack((G[:, tt[0], 0], G[:, tt[1], 1]))
        valid = torch.stack((tt[0] < ln, tt[1] < ln)).view(2, B, 1)
        ig, fg, og = torch.sigmoid(pre[:, :, 0]), torch.sigmoid(pre[:, :, 1]), torch.sigmoid(pre[:, :, 3])
        gg = torch.tanh(pre[:, :, 2])
        c = torch.where(valid, fg * c + ig * gg, zero)
        h = torch.where(valid, og * torch.tanh(c), zero)
        gates = torch.where(valid.unsqueeze(2), torch.stack((ig, fg, gg, og), 2), zero)
        for d in range(2):
            ys[d][tt[d]], cs[d][tt[d]], gs[d][tt[d]] = h[d], c[d], gates[d]
    pack = lambda l: torch.stack([torch.stack(l[0], 1), torch.stack(l[1], 1)], 2)
    return pack(ys), pack(cs), pack(gs)


def dwhh_from_dG(dG, y):
    """dW_hh [2, 4H, H] as the caller of radmmm_lstm_bwd builds it: dW_hh[d] = dG_d^T h_prev (h_{t-1} forward, h_{t+1}
    reverse).  dG [B, T, 2, 4, H], y [B, T, 2, H]."""
    B, T, _, _, H = dG.shape
    hp = torch.zeros_like(y)
    hp[:, 1:, 0] = y[:, :-1, 0]
    hp[:, :-1, 1] = y[:, 1:, 1]
    return torch.einsum("btdgu,btdk->dguk", dG, hp).reshape(2, 4 * H, H)


def bilstm_ref_grads(G, W_hh, lens, dy, dtype=torch.float64, noise=0.0):
    """Forward + autograd backward of sum(y * dy).  -> dict(y, c, gates, dG, dW): dG is the pre-activation gradient the
    kernel leaves in G, dW autograd's gradient of W_hh (== dwhh_from_dG(dG, y))."""
    Gd = G.detach().to(dtype).requires_grad_(True)
    Wd = W_hh.detach().to(dtype).requires_grad_(True)
    y, c, gates = bilstm_ref(Gd, Wd, lens, dtype, noise)
    dG, dW = torch.autograd.grad((y * dy.to(dtype).view_as(y)).sum(), [Gd, Wd])
    return dict(y=y.detach(), c=c.detach(), gates=gates.detach(), dG=dG, dW=dW)


def growth_case(H, T, B=2, seed=0):
    """The gradient-growth set-up: W_hh uniform in +-0.3, N(0, 1) pre-activations with +3 on the forget gate, dy = 1."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(2, 4 * H, H, generator=g) - 0.5) * 0.6
    G = torch.randn(B, T, 2, 4, H, generator=g)
    G[:, :, :, 1] += 3.0
    return G, W, torch.ones(B, T, 2, H)


def expected_lstm_path(lib, B, T, H):
    """What radmmm_lstm_last_path must report for these dimensions: 2 (single cooperative launch) iff the grid of
    ceil(H/8) x 2 x ceil(B/32) workgroups fits the CU slots, the forward gets its per-step operand slots and the switch
    RADMMM_LSTM_PERSISTENT is not 0; else 1 (one launch per step)."""
    sw = os.environ.get("RADMMM_LSTM_PERSISTENT")
    fits = -(-H // 8) * 2 * -(-B // 32) <= lib.radmmm_gemm_cu_slots()
    return 2 if fits and lib.radmmm_lstm_hseq_bytes(B, T, H) > 0 and not (sw is not None and int(sw) == 0) else 1
