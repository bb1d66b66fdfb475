"""The one-product weight gradient of the flow steps' WN convs (radmmm_wgrad_rmh, the one-product instantiation of
csrc/wgrad_rm8.hip's kernel): argument checks without a GPU, the kernel against float64 at its edges (one K step, fewer K
steps than the LDS ring is deep, partial tiles, windows that cross utterances, the length mask), and the two properties the
change rests on -- nothing but the WN convs' weight gradients moves, and the choice is made in forward."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import rel_err, sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rad_mmm_amd", "libradmmm_hip.so")
DEV = "cuda:0"


def test_wgrad_rmh_validates_without_gpu():
    """Null pointers, T = 31, ldg = 40 and splits = 0 return -1 with an error text before any HIP call; the dims cases pass
    dummy non-null addresses, which that path never dereferences."""
    lib = ctypes.CDLL(LIB)
    lib.radmmm_last_error.restype = ctypes.c_char_p
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.radmmm_wgrad_rmh.argtypes = [p, i, p, i, i, i, p, i, p, i, ctypes.c_int64, i, i, i, i, i, f, p]
    d = 0x1000                                                   # never dereferenced

    def call(gy=d, x=d, P=d, ldg=64, ldx=64, B=2, T=32, Mc=64, Nc=64, splits=1):
        return lib.radmmm_wgrad_rmh(gy, ldg, x, ldx, B * T, T, None, 0, P, Nc, Mc * Nc, Mc, Nc, 1, 1, splits, 1.0, None)

    for kw in (dict(gy=None), dict(x=None), dict(P=None)):
        assert call(**kw) == -1
        assert b"wgrad_rmh: null pointer" in lib.radmmm_last_error()
    for kw in (dict(T=31), dict(ldg=40, Mc=40), dict(splits=0)):
        assert call(**kw) == -1
        assert b"wgrad_rmh: bad dims" in lib.radmmm_last_error()


def _contract(gv, xv, taps, dil):
    """[taps, Mc, Nc] float64: sum over the frames f of gv[b, f, m] * xv[b, f + s, n], s = (tap - taps // 2) * dil inside the
    utterance."""
    T = gv.shape[1]
    ref = torch.zeros(taps, gv.shape[2], xv.shape[2], dtype=torch.float64, device=gv.device)
    for tp in range(taps):
        s = (tp - taps // 2) * dil
        lo, hi = max(0, -s), min(T, T - s)
        if hi > lo:
            ref[tp] = torch.einsum("btm,btn->mn", gv[:, lo:hi], xv[:, lo + s:hi + s])
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,Mc,Nc,taps,dil", [
    (4, 64, 256, 256, 1, 1), (3, 96, 320, 288, 5, 2), (2, 160, 1024, 1152, 1, 1), (5, 40, 96, 160, 3, 1), (2, 352, 512, 256, 5, 8),
    (1, 32, 256, 256, 1, 1),          # one K step
    (1, 64, 256, 256, 5, 2),          # two K steps: fewer than the ring is deep
    (2, 96, 160, 1024, 1, 1),         # the end conv: a partial M tile
    (2, 48, 1024, 1152, 1, 1),        # the start conv; the second window crosses the utterance boundary mid-step
])
def test_wgrad_rmh_against_float64(B, T, Mc, Nc, taps, dil):
    """radmmm_wgrad_rmh on the operands of test_wgrad_rm8_fp8_cross_terms (split_f16 of randn * 0.3 at SG = 32, softplus(randn)).
    (i) against the float64 contraction of the dequantised hi planes: 3e-6 of the largest element -- products of fp16 values
    are exact in fp32, only the fp32 accumulation rounds (the bar of radmmm_wgrad_rm at these frame counts);
    (ii) elementwise against the float64 contraction of the fp32 tensors: 2^-10 * (|gy|^T |x|), the hard bound of two
    round-to-nearest fp16 operands, + 3e-6 * max |ref| for the accumulation;
    (iii) with lens: bit-equal to the unmasked call on x * keep;  (iv) two launches: bit-equal."""
    from rad_mmm_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + T)
    gy = (torch.randn(B * T, Mc, generator=g) * 0.3).to(DEV)
    x = torch.nn.functional.softplus(torch.randn(B * T, Nc, generator=g)).to(DEV)
    SG = 32.0
    ldg, ldx = ops.round_up(Mc, 32), ops.round_up(Nc, 32)
    gh, gx = ops.split_f16(gy, Mc, SG, ldg, 2, ops.X8_GRAD_EXP)
    xh, xx = ops.split_f16(x, Nc, 1.0, ldx, 2, ops.X8_ACT_EXP)
    P = ops.wgrad_rmh_slabs(gh, xh, B, T, Mc, Nc, taps, dil, 1.0 / SG).sum(0)
    # (iv)
    assert torch.equal(P, ops.wgrad_rmh_slabs(gh, xh, B, T, Mc, Nc, taps, dil, 1.0 / SG).sum(0))
    # (iii)
    lens = torch.tensor([max(1, T - 7 * b) for b in range(B)], dtype=torch.int32, device=DEV)
    keep = (torch.arange(T, device=DEV)[None] < lens[:, None]).reshape(B * T, 1)
    xmh, _ = ops.split_f16(x * keep, Nc, 1.0, ldx, 2, ops.X8_ACT_EXP)
    Pm = ops.wgrad_rmh_slabs(gh, xh, B, T, Mc, Nc, taps, dil, 1.0 / SG, lens).sum(0)
    Pz = ops.wgrad_rmh_slabs(gh, xmh, B, T, Mc, Nc, taps, dil, 1.0 / SG).sum(0)
    assert torch.equal(Pm, Pz)
    # (i)
    ref_hi = _contract(gh.double()[:, :Mc].view(B, T, Mc) / SG, xh.double()[:, :Nc].view(B, T, Nc), taps, dil)
    err_hi = rel_err(P.double().cpu(), ref_hi.cpu())
    ref_hi_m = _contract(gh.double()[:, :Mc].view(B, T, Mc) / SG, xmh.double()[:, :Nc].view(B, T, Nc), taps, dil)
    err_hi_m = rel_err(Pm.double().cpu(), ref_hi_m.cpu())
    # (ii)
    gv, xv = gy.double().view(B, T, Mc), x.double().view(B, T, Nc)
    ref = _contract(gv, xv, taps, dil)
    bound = 2.0 ** -10 * _contract(gv.abs(), xv.abs(), taps, dil) + 3e-6 * ref.abs().max()
    used = float(((P.double() - ref).abs() / bound).max())          # largest share of its bound that an element uses
    err1 = rel_err(P.double().cpu(), ref.cpu())
    P8 = ops.wgrad_rm8_slabs((gh, gx), ops.X8_GRAD_EXP, (xh, xx), ops.X8_ACT_EXP, B, T, Mc, Nc, taps, dil, 1.0 / SG).sum(0)
    err8 = rel_err(P8.double().cpu(), ref.cpu())
    print(f"wgrad_rmh B={B} T={T} {Mc}x{Nc} taps={taps} dil={dil}: vs hi planes {err_hi:.2e} (masked {err_hi_m:.2e}); vs fp32 "
          f"tensors: one product {err1:.2e}, fp8-cross {err8:.2e}; largest |P - ref| / bound {used:.3f}")
    assert err_hi < 3e-6 and err_hi_m < 3e-6
    assert used <= 1.0


def _decoder_step(golden, products, monkeypatch):
    from oracle import radmmm_oracle as O
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd.decoders import RADMMMFlow
    from rad_mmm_amd.loss import RADMMMLoss
    monkeypatch.setenv("RADMMM_CONVNORM_H3_MIN_ROWS", "0")
    monkeypatch.setenv("RADMMM_F8X_MIN_ROWS", "0")      # keep the FP8-cross scheme on this small batch
    monkeypatch.setenv("RADMMM_PRECISION", "f8x")
    monkeypatch.setenv("RADMMM_WGRAD_PRODUCTS", products)
    g = golden("decoder_cfg2_small.npz")
    kw = {k: (v.item() if v.shape == () else v) for k, v in sub(g, "cfg.").items()}
    cfg = O.DecoderConfig(**kw)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in O.procedural_decoder_state(O.decoder_state_shapes(cfg)).items()}
    dec = RADMMMFlow(use_accent=True, **kw)
    dec.load_state_dict(sd)
    dec.gemm_precision = "f8x"
    dec = dec.to(DEV).train()
    b = {k: torch.from_numpy(np.asarray(v)) for k, v in O.synthetic_batch(int(g["B"]), int(g["T"]), cfg, 1234, bool(g["ragged"])).items()}
    gb = {k: v.to(DEV) for k, v in b.items()}
    mel = gb["mel"].clone().requires_grad_(True)
    ctx = gb["context"].clone().requires_grad_(True)
    sl = SequenceLength(gb["lengths"])
    out = dec(mel, gb["spk"], ctx, sl, gb["f0"], gb["energy"], gb["accent"])
    loss = RADMMMLoss(sigma=1.0, n_group_size=cfg.n_group_size)(out, None, sl, 0)["loss_mel"][0]
    loss.backward()
    res = {"z_mel": out["z_mel"].detach(), "loss": loss.detach(), "grad.mel": mel.grad, "grad.context": ctx.grad}
    for i, ls in enumerate(out["log_s_list"]):
        res[f"log_s.{i}"] = ls.detach()
    return res, {n: p.grad for n, p in dec.named_parameters()}


WN_WEIGHT = re.compile(r"\.affine_param_predictor\.((start|in_layers\.\d+\.conv|res_skip_layers\.\d+)\.weight_[vg]|end\.weight)$")


@pytest.mark.gpu
def test_only_the_wn_weight_gradients_move(golden, monkeypatch):
    """decoder_cfg2_small (B = 2, T = 96) under f8x, forward + NLL + backward with RADMMM_WGRAD_PRODUCTS = 2 and = 1: z, every
    log s, the loss, the gradients of mel and context, every bias gradient and every parameter gradient outside the WN
    convs' weight_v / weight_g / end.weight are bit-equal; those do change, and agree to 5e-4 in L2."""
    r2, g2 = _decoder_step(golden, "2", monkeypatch)
    r1, g1 = _decoder_step(golden, "1", monkeypatch)
    assert r1.keys() == r2.keys() and g1.keys() == g2.keys()
    for k in r2:
        assert torch.equal(r1[k], r2[k]), k
    moved, worst, n_wn = [], 0.0, 0
    for n in g2:
        if WN_WEIGHT.search(n):
            n_wn += 1
            if not torch.equal(g1[n], g2[n]):
                moved.append(n)
            l2 = float((g1[n].double() - g2[n].double()).norm() / g2[n].double().norm())
            worst = max(worst, l2)
            assert l2 < 5e-4, (n, l2)
        else:
            assert torch.equal(g1[n], g2[n]), n
    print(f"one product vs two: {len(moved)} of {n_wn} WN weight gradients differ, worst L2 rel {worst:.2e}")
    assert n_wn > 0 and moved


@pytest.mark.gpu
def test_plan_is_fixed_in_forward(monkeypatch):
    """One flow step (WN width 1024, B = 2, T = 64, f8x): RADMMM_WGRAD_PRODUCTS flipped between forward and backward changes
    nothing -- backward follows the plan made in forward -- while a forward under the other value does."""
    from rad_mmm_amd.common import AffineTransformationLayer
    from rad_mmm_amd.ops import ZLD
    monkeypatch.setenv("RADMMM_F8X_MIN_ROWS", "0")
    B, T, C, D = 2, 64, 160, 96
    torch.manual_seed(11)
    layer = AffineTransformationLayer(C, D, 4, affine_model="wavenet", scaling_fn="tanh", affine_activation="softplus",
                                      n_channels=1024, use_partial_padding=True)
    torch.nn.init.normal_(layer.affine_param_predictor.end.weight, std=0.02)      # (zero would cut every gradient behind it)
    layer = layer.to(DEV)
    z = torch.nn.functional.pad(torch.randn(B * T, C), (0, ZLD - C)).to(DEV)
    cond = torch.randn(B * T, D).to(DEV)
    lens = torch.tensor([T, T - 9], dtype=torch.int32, device=DEV)
    W_eff, b_eff = torch.eye(ZLD, device=DEV), torch.zeros(ZLD, device=DEV)
    mask = (torch.arange(T, device=DEV)[None] < lens[:, None]).float().reshape(B * T, 1)

    def step(fwd, bwd):
        layer.zero_grad(set_to_none=True)
        zc, cc = z.clone().requires_grad_(True), cond.clone().requires_grad_(True)
        monkeypatch.setenv("RADMMM_WGRAD_PRODUCTS", fwd)
        zo, log_s = layer.run(zc, cc, lens, W_eff, b_eff, B, T, precision="f8x")
        scalar = 0.5 * ((zo[:, :C] * mask) ** 2).sum() - (log_s * mask).sum()
        monkeypatch.setenv("RADMMM_WGRAD_PRODUCTS", bwd)
        scalar.backward()
        out = {n: p.grad.clone() for n, p in layer.named_parameters()}
        out["z"], out["cond"] = zc.grad.clone(), cc.grad.clone()
        return out

    same, flipped, other = step("1", "1"), step("1", "2"), step("2", "2")
    for k in same:
        assert torch.equal(same[k], flipped[k]), k
    assert any(not torch.equal(same[k], other[k]) for k in same)
