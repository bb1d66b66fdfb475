"""HiFi-GAN multi-period discriminator and the three GAN losses on the GPU, forward and backward (reference
vocoders/hifigan_models.py: DiscriminatorP, MultiPeriodDiscriminator; loss.py: gan_feature_loss, gan_discriminator_loss,
gan_generator_loss), with ragged batches and no device -> host read.

    mpd = MultiPeriodDiscriminator().cuda()                       # periods 2, 3, 5, 7, 11; the reference's state_dict keys
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = mpd(y, y_hat)               # y, y_hat [B, 1, T]; the reference's nesting and shapes
    loss_d, r_losses, g_losses = mpd.discriminator_loss(y, y_hat.detach(), len_ratios)     # the D step
    loss_fm, loss_gen = mpd.generator_losses(y, y_hat, len_ratios)                          # the G step

Per discriminator (csrc/mpd.hip) real and generated audio run in ONE pass as 2B signals.  A feature map lives
in a channels-last buffer [2B * p sequences][H + 4 rows][C] with two zero rows on either side of every sequence, so the
5-tap window of a strided conv is one contiguous stretch of 5 * C floats and every conv but conv_post is ONE framed
radmmm_rowgemm_f32 launch (a_item_stride set, lda = stride * C_in, K = 5 * C_in) followed by radmmm_mpd_repad (leaky relu
into the next padded buffer).  The first conv reads a small frame matrix that radmmm_mpd_fold_frame cuts from the audio
(reflect tail, fold, windows).  forward() returns strided views of those buffers: zero copies, ordinary differentiable
tensors.  The two fused methods are one autograd node each: the masked reductions run in radmmm_mpd_fm_terms / _finish
(fp64), and the backward walks the layers once for both signals: data gradient = one row GEMM (b_layout 1) +
radmmm_mpd_unframe (the adjoint of the framing in gather form, times the leaky-relu derivative from the saved output),
weight gradient = radmmm_wgrad_f32 over an explicit frame matrix, bias gradient = radmmm_colsum.  No atomics: equal inputs
give equal bits.  Weight norm is folded with torch ops, as HiFiGANGenerator's training does, so autograd carries the
folded weight's gradient on to weight_g / weight_v.

Semantics are the reference's: reflect pad on the right by p - T % p at the padded length T (T must exceed it), fold
x[b, 0, h, w] = audio[b, h * p + w], leaky relu of slope 0.1, no factor 2 in the feature loss.  With len_ratios, item b
counts ceil(len_ratios[b] * H_l) rows of a feature map and ceil(len_ratios[b] * H_post * p) flattened positions of a
discriminator output, the torch expression evaluated on the device in len_ratios' dtype.  The reference's own mask only
broadcasts when some ratio is 1; this module is defined by the formula for any ratios in [0, 1] (a count is read clamped
to its size).  fp32 only; spectral norm and the multi-scale discriminator are not built.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import List, Optional, Sequence

import torch
from torch import nn

from ._lib import RadmmmError, check, f32c, fp32_region, lib, ptr, rowgemm, stream
from .vocoder import fold_weight_norm

LRELU_SLOPE = 0.1
_OPERAND_BYTES = 2 ** 31 - 2 ** 16     # the row GEMM's operands and the kernels' matrices stay below 2 GiB

# test hook: set to a dict to count how often each launch helper runs (which kernels a step launches); None costs one
# comparison per launch
LAUNCHES: Optional[dict] = None


def _count(name: str) -> None:
    if LAUNCHES is not None:
        LAUNCHES[name] = LAUNCHES.get(name, 0) + 1


def _call(name: str, *args) -> None:
    _count(name)
    check(getattr(lib, "radmmm_" + name)(*args, stream()), name)


def _gemm(name: str, **kw) -> None:
    _count(name)
    rowgemm(**kw)


def _wn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.weight_norm(m)


class _Geometry:
    """shapes of one discriminator for B items of T samples"""

    def __init__(self, period: int, channels: Sequence[int], B: int, T: int):
        p = self.p = int(period)
        self.B, self.T = B, T
        n_pad = (p - T % p) % p
        if T <= n_pad:
            raise ValueError(f"DiscriminatorP(period {p}): {T} samples cannot be reflect-padded by {n_pad}")
        self.H0 = (T + n_pad) // p
        self.S = 2 * B * p
        self.C = [int(c) for c in channels]                       # output channels of the five convs
        self.stride = [3, 3, 3, 3, 1]
        self.H = []                                               # output rows of the five convs
        h = self.H0
        for st in self.stride:
            h = (h - 1) // st + 1
            self.H.append(h)
        worst = max(self.S * (self.H[l] + 4) * max(self.C[l], 5 * self.C[l - 1] if l else 8) for l in range(5))
        if 4 * worst > _OPERAND_BYTES:
            raise ValueError(f"DiscriminatorP(period {p}): {B} x {T} samples need a GEMM operand of {4 * worst} bytes, above "
                             f"the row GEMM's limit of {_OPERAND_BYTES}: split the batch")

    def map_sizes(self) -> List[int]:
        """what len_ratios is multiplied with: the rows of the six maps, then the flattened length of the output"""
        return self.H + [self.H[4], self.H[4] * self.p]


def _pack_weights(g: _Geometry, ws: Sequence[torch.Tensor]):
    """reference layouts (folded) -> GEMM layouts.  convs.0 [C1, 1, 5, 1] -> [C1, 8] (taps, zero padded); convs.l
    [Cout, Cin, 5, 1] -> [Cout, 5 * Cin] with k = tap * Cin + ci; conv_post [1, C, 3, 1] -> [3, C]"""
    out = []
    w0 = ws[0].detach().float()
    W0 = torch.zeros(g.C[0], 8, device=w0.device, dtype=torch.float32)
    W0[:, :5] = w0.reshape(g.C[0], 5)
    out.append(W0)
    for l in range(1, 5):
        out.append(ws[2 * l].detach().float()[..., 0].permute(0, 2, 1).reshape(g.C[l], 5 * g.C[l - 1]).contiguous())
    out.append(ws[10].detach().float().reshape(g.C[4], 3).t().contiguous())
    return out


def _disc_forward(g: _Geometry, y: torch.Tensor, y_hat: torch.Tensor, ws: Sequence[torch.Tensor]) -> dict:
    """one discriminator on both signals -> tape: F1 (the first conv's frames), X[0..4] (the padded maps), out [2B, H5, p]"""
    dev = y.device
    S, p, B, T = g.S, g.p, g.B, g.T

    def empty(*shape):
        return torch.empty(*shape, device=dev, dtype=torch.float32)

    W = _pack_weights(g, ws)
    bias = [f32c(ws[2 * l + 1].detach()) for l in range(6)]
    F1 = empty(S * g.H[0], 8)
    _call("mpd_fold_frame", ptr(y), ptr(y_hat), T, ptr(F1), B, T, p, g.H0, g.H[0])
    X = []
    for l in range(5):
        C, H = g.C[l], g.H[l]
        Z = empty(S * H, C)
        if l == 0:
            _gemm("conv", A=F1, lda=8, B=W[0], ldb=8, C=Z, ldc=C, M=S * H, N=C, K=8, T=H, bias=bias[0])
        else:
            Cin, Hin, st = g.C[l - 1], g.H[l - 1], g.stride[l]
            _gemm("conv", **_framed(X[l - 1], S, Hin, Cin, st, W[l], Z, H, C, bias[l]))
        Xl = empty(S, H + 4, C)
        _call("mpd_repad", ptr(Z), C, ptr(Xl), S, H, C, LRELU_SLOPE)
        X.append(Xl)
    out = empty(2 * B, g.H[4], p)
    _call("mpd_conv_post", ptr(X[4]), ptr(W[5]), ptr(bias[5]), ptr(out), 2 * B, p, g.H[4], g.C[4])
    return {"F1": F1, "X": X, "out": out, "W": W}


def _framed(Xin, S, Hin, Cin, st, W, Z, H, C, bias=None) -> dict:
    """the framed row GEMM of one conv: window h' of sequence s is the 5 * Cin floats at padded row st * h'"""
    return dict(A=Xin, lda=st * Cin, a_item_stride=(Hin + 4) * Cin, B=W, ldb=5 * Cin, C=Z, ldc=C, M=S * H, N=C, K=5 * Cin, T=H,
                bias=bias)


def _disc_backward(g: _Geometry, tape: dict, dOut: torch.Tensor, add: Sequence[Optional[torch.Tensor]], want_w: Sequence[bool],
                   want_audio: Sequence[bool]):
    """dOut [2B, H5, p]: gradient of the output; add[l]: gradient of padded map l or None.  -> (weight and bias gradients
    in the reference's layouts, None where not wanted; audio gradients [B, T] of (y, y_hat), None where not wanted)"""
    from .waveglow import _colsum, _wgrad          # (waveglow imports the vocoder module)
    dev = dOut.device
    S, p, B, T = g.S, g.p, g.B, g.T
    X, W = tape["X"], tape["W"]
    grads: List[Optional[torch.Tensor]] = [None] * 12
    if not any(want_w) and not any(want_audio):
        return grads, [None, None]
    half = not any(want_w) and not want_audio[0]
    B2 = B if half else 2 * B
    if half:        # only the generated signal's audio gradient is wanted: walk its half of every buffer alone
        S //= 2
        X = [x[S:] for x in X]
        add = [a[S:] if a is not None else None for a in add]
        dOut = dOut[B:]

    def empty(*shape):
        return torch.empty(*shape, device=dev, dtype=torch.float32)

    C5, H5 = g.C[4], g.H[4]
    if want_w[5]:
        n = int(lib.radmmm_mpd_conv_post_wgrad_parts(B2, p, H5))
        part, dw = empty(n, 3 * C5 + 1), empty(3 * C5 + 1)
        _call("mpd_conv_post_wgrad", ptr(dOut), ptr(X[4]), ptr(part), B2, p, H5, C5)
        _call("colsum_final", ptr(part), ptr(dw), n, 3 * C5 + 1)
        grads[10], grads[11] = dw[:3 * C5].view(3, C5).t().reshape(1, C5, 3, 1), dw[3 * C5:]
    dZ = empty(S * H5, C5)
    _call("mpd_conv_post_dgrad", ptr(dOut), ptr(W[5]), ptr(add[4]), ptr(X[4]), ptr(dZ), B2, p, H5, C5, LRELU_SLOPE)
    for l in range(4, 0, -1):
        C, H, Cin, Hin, st = g.C[l], g.H[l], g.C[l - 1], g.H[l - 1], g.stride[l]
        R = S * H
        if want_w[l]:
            Fr = empty(R, 5 * Cin)
            _call("mpd_frame", ptr(X[l - 1]), ptr(Fr), S, Hin, Cin, H, st)
            _count("wgrad")
            dw = _wgrad(dZ, C, C, Fr, 5 * Cin, 5 * Cin, R, R)[0]
            del Fr
            _count("colsum")
            grads[2 * l], grads[2 * l + 1] = dw.view(C, 5, Cin).permute(0, 2, 1).unsqueeze(-1), _colsum(dZ, C, R, C)
        dF = empty(R, 5 * Cin)
        _gemm("dgrad", A=dZ, lda=C, B=W[l], ldb=5 * Cin, b_layout=1, C=dF, ldc=5 * Cin, M=R, N=5 * Cin, K=C, T=H)
        dZ = empty(S * Hin, Cin)
        _call("mpd_unframe", ptr(dF), ptr(add[l - 1]), ptr(X[l - 1]), ptr(dZ), S, Hin, Cin, H, st, LRELU_SLOPE)
        del dF
    C, H = g.C[0], g.H[0]
    R = S * H
    if want_w[0]:
        _count("wgrad")
        dw = _wgrad(dZ, C, C, tape["F1"], 8, 8, R, R)[0]
        _count("colsum")
        grads[0], grads[1] = dw[:, :5].reshape(C, 1, 5, 1), _colsum(dZ, C, R, C)
    g_audio: List[Optional[torch.Tensor]] = [None, None]
    if any(want_audio):
        dF = empty(R, 8)
        _gemm("dgrad_audio", A=dZ, lda=C, B=W[0], ldb=8, b_layout=1, C=dF, ldc=8, M=R, N=8, K=C, T=H)
        for sig in range(2):
            if want_audio[sig]:
                g_audio[sig] = empty(B, T)
                _call("mpd_unfold_audio", ptr(dF), ptr(g_audio[sig]), T, B, T, p, g.H0, H, 0 if half else sig)
    return grads, g_audio


def _views(g: _Geometry, tape_bufs: Sequence[torch.Tensor]):
    """the six buffers of one discriminator -> (y_d_r, y_d_g, fmap_r, fmap_g): strided views, no copies"""
    B, p = g.B, g.p
    fm = ([], [])
    for l in range(5):
        v = tape_bufs[l].view(2, B, p, g.H[l] + 4, g.C[l])[:, :, :, 2:2 + g.H[l], :].permute(0, 1, 4, 3, 2)   # [2, B, C, H, p]
        fm[0].append(v[0])
        fm[1].append(v[1])
    out = tape_bufs[5].view(2, B, 1, g.H[4], p)
    fm[0].append(out[0])
    fm[1].append(out[1])
    return out[0].reshape(B, g.H[4] * p), out[1].reshape(B, g.H[4] * p), fm[0], fm[1]


class _MPDFn(torch.autograd.Function):
    """The multi-period discriminator as one autograd node.  Inputs: mode, the geometries, y [B, T], y_hat [B, T], cnt
    (int32 [discriminators, 7, B] or None), then per discriminator (weight, bias) of its six convs, reference layouts, weight
    norm already folded.  mode "views": the outputs are the buffers forward() cuts its views from (per discriminator the
    five padded maps and the output).  mode "disc": (loss, r_losses [n], g_losses [n]).  mode "gen": (loss_fm, loss_gen)."""

    @staticmethod
    def forward(ctx, mode, geos, y, y_hat, cnt, *weights):
        dev = y.device
        y, y_hat = f32c(y.detach()), f32c(y_hat.detach())
        n = len(geos)
        tapes = [_disc_forward(g, y, y_hat, weights[12 * i:12 * i + 12]) for i, g in enumerate(geos)]
        ctx.mode, ctx.geos, ctx.has_cnt = mode, geos, cnt is not None
        ctx.set_materialize_grads(False)
        keep = [b for t in tapes for b in (t["F1"], *t["X"], t["out"], *t["W"])]      # 13 per discriminator
        if mode == "views":
            ctx.save_for_backward(*keep)
            return tuple(b for t in tapes for b in (*t["X"], t["out"]))
        res = torch.empty(n, 4, device=dev, dtype=torch.float32)
        norm = torch.empty(n, 8, device=dev, dtype=torch.float64)
        for i, (g, t) in enumerate(zip(geos, tapes)):
            ci = cnt[i] if cnt is not None else None
            with_fm = mode == "gen"
            Cs, Hs = g.C + [1], g.H + [g.H[4]]
            offs = [0]
            for l in range(6):
                offs.append(offs[-1] + (int(lib.radmmm_mpd_fm_terms_parts(g.B, g.p, Hs[l], Cs[l])) if with_fm else 0))
            part = torch.empty(max(offs[-1], 1), device=dev, dtype=torch.float32)
            if with_fm:
                for l in range(6):
                    src = t["X"][l] if l < 5 else t["out"]
                    _call("mpd_fm_terms", ptr(src), ptr(ci[l]) if ci is not None else None, ptr(part[offs[l]:]), g.B, g.p,
                          Hs[l], Cs[l], int(l < 5))
            i32 = ctypes.c_int32
            _call("mpd_finish", ptr(part), (i32 * 7)(*offs), (i32 * 6)(*Cs), (i32 * 6)(*Hs), ptr(t["out"]), ptr(ci),
                  ptr(res[i]), ptr(norm[i]), g.B, g.p)
        ctx.save_for_backward(*keep, norm, *([cnt] if cnt is not None else []))
        if mode == "disc":
            r, gl = res[:, 1].clone(), res[:, 2].clone()
            return (r + gl).sum(), r, gl
        return res[:, 0].sum(), res[:, 3].sum()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        geos, mode = ctx.geos, ctx.mode
        n = len(geos)
        saved = list(ctx.saved_tensors)
        tapes = [{"F1": saved[13 * i], "X": saved[13 * i + 1:13 * i + 6], "out": saved[13 * i + 6], "W": saved[13 * i + 7:13 * i + 13]}
                 for i in range(n)]
        norm = saved[13 * n] if mode != "views" else None
        cnt = saved[13 * n + 1] if ctx.has_cnt else None
        dev = tapes[0]["out"].device
        want_audio = [ctx.needs_input_grad[2], ctx.needs_input_grad[3]]
        wneed = ctx.needs_input_grad[5:]
        if mode != "views":
            zero = torch.zeros(n, device=dev, dtype=torch.float32)
            if mode == "disc":      # loss = sum (r + g): d/d r_i = g_loss + g_r[i]
                gl, gr, gg = (f32c(x) if x is not None else None for x in gouts)
                base = gl if gl is not None else zero[0]
                up = torch.stack([zero, base + (gr if gr is not None else zero), base + (gg if gg is not None else zero), zero], 1)
            else:
                gfm, ggen = (f32c(x) if x is not None else None for x in gouts)
                up = torch.stack([zero + (gfm if gfm is not None else 0.0), zero, zero, zero + (ggen if ggen is not None else 0.0)], 1)
            up = up.contiguous()
        out_grads: List[Optional[torch.Tensor]] = []
        audio = [None, None]
        for i, (g, t) in enumerate(zip(geos, tapes)):
            want_w = [bool(wneed[12 * i + 2 * l] or wneed[12 * i + 2 * l + 1]) for l in range(6)]
            if mode == "views":
                gb = gouts[6 * i:6 * i + 6]
                add = [f32c(x) if x is not None else None for x in gb[:5]]
                dOut = f32c(gb[5]) if gb[5] is not None else torch.zeros_like(t["out"])
            else:
                ci = cnt[i] if cnt is not None else None
                add = [None] * 5
                if mode == "gen":
                    for l in range(5):
                        add[l] = torch.empty_like(t["X"][l])
                        _call("mpd_fm_grad", ptr(t["X"][l]), ptr(ci[l]) if ci is not None else None, ptr(norm[i, l:]),
                              ptr(up[i]), ptr(add[l]), g.B, g.p, g.H[l], g.C[l])
                dOut = torch.empty_like(t["out"])
                _call("mpd_out_grad", ptr(t["out"]), ptr(ci), ptr(norm[i]), ptr(up[i]), ptr(dOut), g.B, g.p, g.H[4])
            grads, ga = _disc_backward(g, t, dOut, add, want_w, want_audio)
            out_grads += [gr if wneed[12 * i + k] else None for k, gr in enumerate(grads)]
            for sig in range(2):
                if ga[sig] is not None:
                    audio[sig] = ga[sig] if audio[sig] is None else audio[sig].add_(ga[sig])
        return (None, None, audio[0], audio[1], None, *out_grads)


class DiscriminatorP(nn.Module):
    """DiscriminatorP(period) of hifigan_models.py:249-283 with the reference's parameter names: convs.N.weight_g / weight_v
    [Cout, Cin, 5, 1] / bias, conv_post.* with a (3, 1) kernel, weight norm over dim 0.  channels: the five convs' widths
    (multiples of 4; narrow models for tests).  forward(y, y_hat) -> (y_d_r, y_d_g, fmap_r, fmap_g)."""

    def __init__(self, period: int, channels: Sequence[int] = (32, 128, 512, 1024, 1024), use_spectral_norm: bool = False):
        super().__init__()
        if use_spectral_norm:
            raise NotImplementedError("DiscriminatorP: spectral norm is not built (the multi-period discriminator never uses it)")
        if len(channels) != 5 or any(int(c) <= 0 or int(c) % 4 for c in channels):
            raise ValueError(f"DiscriminatorP: channels must be five positive multiples of 4, got {tuple(channels)}")
        if int(period) < 1:
            raise ValueError(f"DiscriminatorP: period {period}")
        self.period, self.channels = int(period), tuple(int(c) for c in channels)
        cin, convs = 1, []
        for i, c in enumerate(self.channels):
            convs.append(_wn(nn.Conv2d(cin, c, (5, 1), (3 if i < 4 else 1, 1), padding=(2, 0))))
            cin = c
        self.convs = nn.ModuleList(convs)
        self.conv_post = _wn(nn.Conv2d(cin, 1, (3, 1), 1, padding=(1, 0)))

    def _layers(self):
        return list(self.convs) + [self.conv_post]

    def remove_weight_norm(self):
        for m in self._layers():
            if "weight_g" in m._parameters:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    nn.utils.remove_weight_norm(m)

    def apply_weight_norm(self):
        for m in self._layers():
            if "weight_g" not in m._parameters:
                _wn(m)

    def _weights(self) -> List[torch.Tensor]:
        """(weight, bias) of the six convs, reference layouts; a weight-normed conv's weight is folded with torch ops, so
        autograd carries the node's gradient of the folded weight on to weight_g and weight_v"""
        out = []
        for m in self._layers():
            out.append(fold_weight_norm(m.weight_v.float(), m.weight_g.float()) if "weight_g" in m._parameters else m.weight)
            out.append(m.bias)
        return out

    def forward(self, y, y_hat):
        r, g_, fr, fg = _run([self], "views", y, y_hat, None)
        return r[0], g_[0], fr[0], fg[0]


def _audio(y: torch.Tensor, y_hat: torch.Tensor):
    if not (isinstance(y, torch.Tensor) and isinstance(y_hat, torch.Tensor) and y.is_cuda and y_hat.is_cuda):
        raise RadmmmError("MultiPeriodDiscriminator needs GPU tensors (there is no CPU path)")
    if y.shape != y_hat.shape or y.dim() != 3 or y.shape[1] != 1:
        raise ValueError(f"MultiPeriodDiscriminator: y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must both be [B, 1, T]")
    return y.reshape(y.shape[0], y.shape[2]), y_hat.reshape(y.shape[0], y.shape[2])


def _counts(len_ratios, geos: Sequence, B: int, dev: torch.device) -> Optional[torch.Tensor]:
    """the reference's (len_ratios * size).ceil().long() for every size in map_sizes() of every discriminator (_Geometry or
    _GeometryS), in len_ratios' dtype on the device, as int32 [discriminators, sizes, B]: 7 sizes for the multi-period, 9 for
    the multi-scale discriminator (the kernels read it clamped to [0, size])"""
    if len_ratios is None:
        return None
    if not (isinstance(len_ratios, torch.Tensor) and len_ratios.is_cuda):
        host = torch.as_tensor(len_ratios)
        if not host.is_floating_point():
            host = host.float()
        len_ratios = host.reshape(-1).pin_memory().to(dev, non_blocking=True)
    r = len_ratios.reshape(-1)
    if r.numel() != B:
        raise ValueError(f"len_ratios has {r.numel()} entries for {B} items")
    return torch.stack([torch.stack([(r * size).ceil().to(torch.int32) for size in g.map_sizes()]) for g in geos])


@fp32_region
def _run(discs: Sequence[DiscriminatorP], mode: str, y, y_hat, len_ratios):
    y2, yh2 = _audio(y, y_hat)
    B, T = y2.shape
    geos = [_Geometry(d.period, d.channels, B, T) for d in discs]         # every refusal comes before the first launch
    for d in discs:
        if any(p_.dtype != torch.float32 for p_ in d.parameters()):
            raise RadmmmError("MultiPeriodDiscriminator is fp32 only")
    cnt = _counts(len_ratios, geos, B, y2.device) if mode != "views" else None
    weights = [w for d in discs for w in d._weights()]
    outs = _MPDFn.apply(mode, geos, y2, yh2, cnt, *weights)
    if mode != "views":
        return outs
    rs, gs, frs, fgs = [], [], [], []
    for i, g in enumerate(geos):
        r, g_, fr, fg = _views(g, outs[6 * i:6 * i + 6])
        rs.append(r), gs.append(g_), frs.append(fr), fgs.append(fg)
    return rs, gs, frs, fgs


class MultiPeriodDiscriminator(nn.Module):
    """MultiPeriodDiscriminator of hifigan_models.py:286-310; state_dict keys discriminators.N.convs.M.{weight_g, weight_v,
    bias} and discriminators.N.conv_post.*, so the `mpd` entry of an upstream checkpoint loads with load_state_dict."""

    def __init__(self, periods: Sequence[int] = (2, 3, 5, 7, 11), channels: Sequence[int] = (32, 128, 512, 1024, 1024)):
        super().__init__()
        self.discriminators = nn.ModuleList(DiscriminatorP(p, channels) for p in periods)

    def remove_weight_norm(self):
        for d in self.discriminators:
            d.remove_weight_norm()

    def apply_weight_norm(self):
        for d in self.discriminators:
            d.apply_weight_norm()

    def forward(self, y, y_hat):
        """y, y_hat [B, 1, T] -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) as the reference nests them: outputs [B, H_post * p],
        feature maps [B, C, H_l, p], all strided views of the kernels' buffers"""
        return _run(list(self.discriminators), "views", y, y_hat, None)

    def discriminator_loss(self, y, y_hat, len_ratios=None):
        """gan_discriminator_loss(*forward(y, y_hat)[:2], len_ratios) -> (loss, r_losses, g_losses); the per-discriminator
        terms are device tensors [n], nothing is read back"""
        return _run(list(self.discriminators), "disc", y, y_hat, len_ratios)

    def generator_losses(self, y, y_hat, len_ratios=None):
        """(gan_feature_loss(fmap_rs, fmap_gs, len_ratios), gan_generator_loss(y_d_gs, len_ratios)[0])"""
        return _run(list(self.discriminators), "gen", y, y_hat, len_ratios)


def load_mpd(path: str, device="cuda") -> MultiPeriodDiscriminator:
    """the `mpd` entry of an upstream do_* checkpoint -> MultiPeriodDiscriminator on `device`"""
    ckpt = torch.load(path, map_location="cpu")
    if "mpd" not in ckpt:
        raise KeyError(f"{path} has no 'mpd' entry (keys: {sorted(ckpt)[:8]})")
    mpd = MultiPeriodDiscriminator()
    mpd.load_state_dict(ckpt["mpd"])
    return mpd.to(device)


# ---------------------------------------------------------------------------------------------------------------------------
# The multi-scale discriminator (hifigan_models.py: DiscriminatorS, MultiScaleDiscriminator)
#
# One member sees S = 2B sequences, s = sig * B + b.  A feature map is a channels-last buffer [S][pad + H + pad][C] padded
# for the conv that reads it: 20 for the five grouped 41-tap convs (csrc/msd.hip: one launch per layer, straight into the
# next padded buffer), 2 for the dense 5-tap conv and for conv_post, which are what the multi-period discriminator's fifth
# conv and conv_post are with p = 1.  The first conv is a 16-column frame matrix plus a plain row GEMM.  A spectral-norm
# member in training mode runs two passes of B sequences, one weight set each, into the halves of the same buffers.
MSD_KERNELS = (15, 41, 41, 41, 41, 41, 5)
MSD_STRIDES = (1, 2, 2, 4, 4, 1, 1)
_MSD_PAD = (20, 20, 20, 20, 20, 2, 2)          # of the map conv l WRITES


def fold_spectral_norm(weight_orig: torch.Tensor, u: torch.Tensor, v: torch.Tensor, training: bool, eps: float = 1e-12):
    """what torch.nn.utils.spectral_norm (dim 0, one power iteration) computes per module call, from torch ops under
    autograd: in training mode v <- normalize(W^T u), u <- normalize(W v) IN PLACE under no_grad, then W / sigma with
    sigma = u . (W v) on clones of the updated vectors; in eval mode the buffers stay and are used as they are"""
    w_mat = weight_orig.flatten(1)
    if training:
        with torch.no_grad():
            v.copy_(nn.functional.normalize(torch.mv(w_mat.t(), u), dim=0, eps=eps))
            u.copy_(nn.functional.normalize(torch.mv(w_mat, v), dim=0, eps=eps))
        u, v = u.clone(), v.clone()
    return weight_orig / torch.dot(u, torch.mv(w_mat, v))


class _GeometryS:
    """shapes of one DiscriminatorS for B items of T samples"""

    def __init__(self, channels: Sequence[int], groups: Sequence[int], B: int, T: int):
        if T < 1:
            raise ValueError(f"DiscriminatorS: {T} samples are too short")
        self.B, self.T, self.S, self.p = B, T, 2 * B, 1
        self.C, self.G = [int(c) for c in channels], [int(g) for g in groups]
        self.H = []
        h = T
        for st in MSD_STRIDES:
            h = (h - 1) // st + 1
            self.H.append(h)
        worst = max([self.S * T * 16] + [self.S * (self.H[l] + 2 * _MSD_PAD[l]) * self.C[l] for l in range(7)]
                    + [self.S * self.H[6] * 5 * self.C[5]])
        if 4 * worst > _OPERAND_BYTES:
            raise ValueError(f"DiscriminatorS: {B} x {T} samples need an operand of {4 * worst} bytes, above the kernels' limit "
                             f"of {_OPERAND_BYTES}: split the batch")

    def map_sizes(self) -> List[int]:
        """what len_ratios is multiplied with: the rows of the eight maps, then the length of the output"""
        return self.H + [self.H[6], self.H[6]]


def _pack_weights_s(g: _GeometryS, ws: Sequence[torch.Tensor]):
    """reference layouts (folded) -> kernel layouts.  convs.0 [C0, 1, 15] -> [C0, 16]; grouped convs.l [Cout, Cin_g, 41] ->
    [G][Cout_g][41 * Cin_g], kk = tap * Cin_g + ci; convs.6 [C6, C5, 5] -> [C6, 5 * C5]; conv_post [1, C6, 3] -> [3, C6]"""
    w0 = ws[0].detach().float()
    W0 = torch.zeros(g.C[0], 16, device=w0.device, dtype=torch.float32)
    W0[:, :15] = w0.reshape(g.C[0], 15)
    out = [W0]
    for l in range(1, 7):
        out.append(ws[2 * l].detach().float().permute(0, 2, 1).contiguous())
    out.append(ws[14].detach().float().reshape(g.C[6], 3).t().contiguous())
    return out


def _gconv_dims(g: _GeometryS, l: int):
    return (g.H[l - 1], g.H[l], g.G[l], g.C[l - 1] // g.G[l], g.C[l] // g.G[l], MSD_KERNELS[l], MSD_STRIDES[l])


def _s_forward_pass(g: _GeometryS, tape: dict, s0: int, n: int, ws: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """sequences [s0, s0 + n) of one member through its eight convs with one weight set -> the packed weights"""
    dev = tape["out"].device
    T, X = g.T, tape["X"]
    W = _pack_weights_s(g, ws)
    bias = [f32c(ws[2 * l + 1].detach()) for l in range(8)]
    Z = torch.empty(n * T, g.C[0], device=dev, dtype=torch.float32)
    _gemm("conv", A=tape["F1"][s0 * T:], lda=16, B=W[0], ldb=16, C=Z, ldc=g.C[0], M=n * T, N=g.C[0], K=16, T=T, bias=bias[0])
    _call("msd_repad", ptr(Z), g.C[0], ptr(X[0][s0:]), n, T, g.C[0], _MSD_PAD[0], LRELU_SLOPE)
    for l in range(1, 6):
        _call("msd_gconv_fwd", ptr(X[l - 1][s0:]), ptr(W[l]), ptr(bias[l]), ptr(X[l][s0:]), n, *_gconv_dims(g, l), _MSD_PAD[l],
              LRELU_SLOPE)
    Z = torch.empty(n * g.H[6], g.C[6], device=dev, dtype=torch.float32)
    _gemm("conv", **_framed(X[5][s0:], n, g.H[5], g.C[5], 1, W[6], Z, g.H[6], g.C[6], bias[6]))
    _call("mpd_repad", ptr(Z), g.C[6], ptr(X[6][s0:]), n, g.H[6], g.C[6], LRELU_SLOPE)
    _call("mpd_conv_post", ptr(X[6][s0:]), ptr(W[7]), ptr(bias[7]), ptr(tape["out"][s0:]), n, 1, g.H[6], g.C[6])
    return W


def _s_forward(g: _GeometryS, y: torch.Tensor, ldy: int, y_hat: torch.Tensor, weight_sets) -> dict:
    """one member on both signals -> tape: F1 (the first conv's frames), X[0..6] (the padded maps), out [2B, H7, 1], W (one
    packed weight list per pass).  One weight set: one pass of 2B; two: the real half with the first, the generated half
    with the second"""
    dev = y.device
    B, S, T = g.B, g.S, g.T
    tape = {"F1": torch.empty(S * T, 16, device=dev, dtype=torch.float32),
            "X": [torch.empty(S, g.H[l] + 2 * _MSD_PAD[l], g.C[l], device=dev, dtype=torch.float32) for l in range(7)],
            "out": torch.empty(S, g.H[6], 1, device=dev, dtype=torch.float32)}
    _call("msd_frame15", ptr(y), ptr(y_hat), ldy, ptr(tape["F1"]), B, T)
    if len(weight_sets) == 1:
        tape["W"] = [_s_forward_pass(g, tape, 0, S, weight_sets[0])]
    else:
        tape["W"] = [_s_forward_pass(g, tape, sig * B, B, weight_sets[sig]) for sig in range(2)]
    return tape


def _s_backward_pass(g: _GeometryS, tape: dict, W, s0: int, n: int, dOut, add, want_w: Sequence[bool], want_audio: Sequence[bool]):
    """sequences [s0, s0 + n) backwards with the weight set W.  want_audio: per signal of THIS range (n = 2B: both; n = B:
    one entry).  -> (16 weight and bias gradients in the reference's layouts or None, audio gradients [B, T] per signal)"""
    from .waveglow import _colsum, _wgrad          # (waveglow imports the vocoder module)
    dev = dOut.device
    B, T = g.B, g.T
    X = [x[s0:s0 + n] for x in tape["X"]]
    add = [a[s0:s0 + n] if a is not None else None for a in add]
    dOut = dOut[s0:s0 + n]
    grads: List[Optional[torch.Tensor]] = [None] * 16

    def empty(*shape):
        return torch.empty(*shape, device=dev, dtype=torch.float32)

    def below(l):                                   # is anything under conv l still wanted?
        return any(want_w[:l]) or any(want_audio)

    C6, H6, C5, H5 = g.C[6], g.H[6], g.C[5], g.H[5]
    if want_w[7]:
        np_ = int(lib.radmmm_mpd_conv_post_wgrad_parts(n, 1, H6))
        part, dw = empty(np_, 3 * C6 + 1), empty(3 * C6 + 1)
        _call("mpd_conv_post_wgrad", ptr(dOut), ptr(X[6]), ptr(part), n, 1, H6, C6)
        _call("colsum_final", ptr(part), ptr(dw), np_, 3 * C6 + 1)
        grads[14], grads[15] = dw[:3 * C6].view(3, C6).t().reshape(1, C6, 3), dw[3 * C6:]
    if not below(7):
        return grads, [None] * len(want_audio)
    dZ = empty(n * H6, C6)
    _call("mpd_conv_post_dgrad", ptr(dOut), ptr(W[7]), ptr(add[6]), ptr(X[6]), ptr(dZ), n, 1, H6, C6, LRELU_SLOPE)
    R = n * H6
    if want_w[6]:
        Fr = empty(R, 5 * C5)
        _call("mpd_frame", ptr(X[5]), ptr(Fr), n, H5, C5, H6, 1)
        _count("wgrad")
        dw = _wgrad(dZ, C6, C6, Fr, 5 * C5, 5 * C5, R, R)[0]
        del Fr
        _count("colsum")
        grads[12], grads[13] = dw.view(C6, 5, C5).permute(0, 2, 1), _colsum(dZ, C6, R, C6)
    if not below(6):
        return grads, [None] * len(want_audio)
    dF = empty(R, 5 * C5)
    _gemm("dgrad", A=dZ, lda=C6, B=W[6], ldb=5 * C5, b_layout=1, C=dF, ldc=5 * C5, M=R, N=5 * C5, K=C6, T=H6)
    dZ = empty(n * H5, C5)
    _call("mpd_unframe", ptr(dF), ptr(add[5]), ptr(X[5]), ptr(dZ), n, H5, C5, H6, 1, LRELU_SLOPE)
    del dF
    for l in range(5, 0, -1):
        Hin, Hout, G, cig, cog, k, st = dims = _gconv_dims(g, l)
        if want_w[l]:
            ns, cols = int(lib.radmmm_msd_gconv_wgrad_splits(n, Hout, G, k)), g.C[l] * k * cig
            P, dw = empty(ns, cols), empty(cols)
            _call("msd_gconv_wgrad", ptr(dZ), ptr(X[l - 1]), ptr(P), n, *dims)
            _call("colsum_final", ptr(P), ptr(dw), ns, cols)
            del P
            _count("colsum")
            grads[2 * l], grads[2 * l + 1] = dw.view(g.C[l], k, cig).permute(0, 2, 1), _colsum(dZ, g.C[l], n * Hout, g.C[l])
        if not below(l):
            return grads, [None] * len(want_audio)
        dX = empty(n * Hin, g.C[l - 1])
        _call("msd_gconv_dgrad", ptr(dZ), ptr(W[l]), ptr(add[l - 1]), ptr(X[l - 1]), ptr(dX), n, *dims, LRELU_SLOPE)
        dZ = dX
    C0, R = g.C[0], n * T
    if want_w[0]:
        _count("wgrad")
        dw = _wgrad(dZ, C0, C0, tape["F1"][s0 * T:], 16, 16, R, R)[0]
        _count("colsum")
        grads[0], grads[1] = dw[:, :15].reshape(C0, 1, 15), _colsum(dZ, C0, R, C0)
    g_audio: List[Optional[torch.Tensor]] = [None] * len(want_audio)
    if any(want_audio):
        dF = empty(R, 16)
        _gemm("dgrad_audio", A=dZ, lda=C0, B=W[0], ldb=16, b_layout=1, C=dF, ldc=16, M=R, N=16, K=C0, T=T)
        for j, want in enumerate(want_audio):
            if want:
                g_audio[j] = empty(B, T)
                _call("msd_unframe15", ptr(dF[j * B * T:]), ptr(g_audio[j]), T, B, T)
    return grads, g_audio


def _s_backward(g: _GeometryS, tape: dict, dOut, add, want_w, want_audio):
    """want_w: per pass, per conv.  -> (per pass 16 gradients, audio gradients of (y, y_hat))"""
    B, S = g.B, g.S
    if len(tape["W"]) == 1:
        if not any(want_w[0]) and not want_audio[0]:
            if not want_audio[1]:
                return [[None] * 16], [None, None]
            # only the generated signal's audio gradient is wanted: walk its half of every buffer alone
            gr, ga = _s_backward_pass(g, tape, tape["W"][0], B, B, dOut, add, want_w[0], [True])
            return [gr], [None, ga[0]]
        gr, ga = _s_backward_pass(g, tape, tape["W"][0], 0, S, dOut, add, want_w[0], want_audio)
        return [gr], ga
    grads, audio = [], []
    for sig in range(2):
        if any(want_w[sig]) or want_audio[sig]:
            gr, ga = _s_backward_pass(g, tape, tape["W"][sig], sig * B, B, dOut, add, want_w[sig], [want_audio[sig]])
        else:
            gr, ga = [None] * 16, [None]
        grads.append(gr)
        audio.append(ga[0])
    return grads, audio


def _views_s(g: _GeometryS, bufs: Sequence[torch.Tensor]):
    """the eight buffers of one member -> (y_d_r, y_d_g, fmap_r, fmap_g): strided views, no copies"""
    B = g.B
    fm = ([], [])
    for l in range(7):
        pad, H = _MSD_PAD[l], g.H[l]
        v = bufs[l].view(2, B, H + 2 * pad, g.C[l])[:, :, pad:pad + H, :].permute(0, 1, 3, 2)        # [2, B, C, H]
        fm[0].append(v[0])
        fm[1].append(v[1])
    out = bufs[7].view(2, B, 1, g.H[6])
    fm[0].append(out[0])
    fm[1].append(out[1])
    return out[0].reshape(B, g.H[6]), out[1].reshape(B, g.H[6]), fm[0], fm[1]


class _MSDFn(torch.autograd.Function):
    """Members of the multi-scale discriminator as one autograd node.  Inputs: mode, the geometries, passes (weight sets per
    member: 1, or 2 for a spectral-norm member in training mode), y [B, T], y_hat [B, T], cnt (int32 [members, 9, B] or None),
    then per member and pass (weight, bias) of its eight convs, reference layouts, norms already folded.  Member i > 0 sees the
    audio pooled i times (radmmm_msd_avgpool).  mode "views": the outputs are per member the seven padded maps and the output.
    mode "disc": (loss, r_losses [n], g_losses [n]).  mode "gen": (loss_fm, loss_gen)."""

    @staticmethod
    def forward(ctx, mode, geos, passes, y, y_hat, cnt, *weights):
        dev = y.device
        y, y_hat = f32c(y.detach()), f32c(y_hat.detach())
        n = len(geos)
        tapes, at = [], 0
        a, ah, ld = y, y_hat, y.shape[1]
        for i, g in enumerate(geos):
            if i:
                pooled = torch.empty(2 * g.B, g.T, device=dev, dtype=torch.float32)
                _call("msd_avgpool", ptr(a), ptr(ah), ld, ptr(pooled), g.B, geos[i - 1].T)
                a, ah, ld = pooled[:g.B], pooled[g.B:], g.T
            tapes.append(_s_forward(g, a, ld, ah, [weights[at + 16 * j:at + 16 * j + 16] for j in range(passes[i])]))
            at += 16 * passes[i]
        ctx.mode, ctx.geos, ctx.passes, ctx.has_cnt = mode, geos, passes, cnt is not None
        ctx.set_materialize_grads(False)
        keep = [b for t in tapes for b in (t["F1"], *t["X"], t["out"], *[w for W in t["W"] for w in W])]
        if mode == "views":
            ctx.save_for_backward(*keep)
            return tuple(b for t in tapes for b in (*t["X"], t["out"]))
        res = torch.empty(n, 4, device=dev, dtype=torch.float32)
        norm = torch.empty(n, 10, device=dev, dtype=torch.float64)
        for i, (g, t) in enumerate(zip(geos, tapes)):
            ci = cnt[i] if cnt is not None else None
            with_fm = mode == "gen"
            Cs, Hs = g.C + [1], g.H + [g.H[6]]
            offs = [0]
            for l in range(8):
                offs.append(offs[-1] + (int(lib.radmmm_mpd_fm_terms_parts(g.B, 1, Hs[l], Cs[l])) if with_fm else 0))
            part = torch.empty(max(offs[-1], 1), device=dev, dtype=torch.float32)
            if with_fm:
                for l in range(8):
                    src = t["X"][l] if l < 7 else t["out"]
                    _call("msd_fm_terms", ptr(src), ptr(ci[l]) if ci is not None else None, ptr(part[offs[l]:]), g.B, Hs[l], Cs[l],
                          _MSD_PAD[l] if l < 7 else -1)
            i32 = ctypes.c_int32
            _call("msd_finish", ptr(part), (i32 * 9)(*offs), (i32 * 8)(*Cs), (i32 * 8)(*Hs), ptr(t["out"]), ptr(ci), ptr(res[i]),
                  ptr(norm[i]), g.B)
        ctx.save_for_backward(*keep, norm, *([cnt] if cnt is not None else []))
        if mode == "disc":
            r, gl = res[:, 1].clone(), res[:, 2].clone()
            return (r + gl).sum(), r, gl
        return res[:, 0].sum(), res[:, 3].sum()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        geos, mode, passes = ctx.geos, ctx.mode, ctx.passes
        n = len(geos)
        saved = list(ctx.saved_tensors)
        tapes, at = [], 0
        for i in range(n):
            t = {"F1": saved[at], "X": saved[at + 1:at + 8], "out": saved[at + 8],
                 "W": [saved[at + 9 + 8 * j:at + 17 + 8 * j] for j in range(passes[i])]}
            at += 9 + 8 * passes[i]
            tapes.append(t)
        norm = saved[at] if mode != "views" else None
        cnt = saved[at + 1] if ctx.has_cnt else None
        dev = tapes[0]["out"].device
        want_audio = [ctx.needs_input_grad[3], ctx.needs_input_grad[4]]
        wneed = ctx.needs_input_grad[6:]
        if mode != "views":
            zero = torch.zeros(n, device=dev, dtype=torch.float32)
            if mode == "disc":      # loss = sum (r + g): d/d r_i = g_loss + g_r[i]
                gl, gr, gg = (f32c(x) if x is not None else None for x in gouts)
                base = gl if gl is not None else zero[0]
                up = torch.stack([zero, base + (gr if gr is not None else zero), base + (gg if gg is not None else zero), zero], 1)
            else:
                gfm, ggen = (f32c(x) if x is not None else None for x in gouts)
                up = torch.stack([zero + (gfm if gfm is not None else 0.0), zero, zero, zero + (ggen if ggen is not None else 0.0)], 1)
            up = up.contiguous()
        out_grads: List[Optional[torch.Tensor]] = []
        member_audio = []
        wat = 0
        for i, (g, t) in enumerate(zip(geos, tapes)):
            want_w = [[bool(wneed[wat + 16 * j + 2 * l] or wneed[wat + 16 * j + 2 * l + 1]) for l in range(8)] for j in range(passes[i])]
            if mode == "views":
                gb = gouts[8 * i:8 * i + 8]
                add = [f32c(x) if x is not None else None for x in gb[:7]]
                dOut = f32c(gb[7]) if gb[7] is not None else torch.zeros_like(t["out"])
            else:
                ci = cnt[i] if cnt is not None else None
                add = [None] * 7
                if mode == "gen":
                    for l in range(7):
                        add[l] = torch.empty_like(t["X"][l])
                        _call("msd_fm_grad", ptr(t["X"][l]), ptr(ci[l]) if ci is not None else None, ptr(norm[i, l:]), ptr(up[i]),
                              ptr(add[l]), g.B, g.H[l], g.C[l], _MSD_PAD[l])
                dOut = torch.empty_like(t["out"])
                _call("msd_out_grad", ptr(t["out"]), ptr(ci), ptr(norm[i]), ptr(up[i]), ptr(dOut), g.B, g.H[6])
            grads, ga = _s_backward(g, t, dOut, add, want_w, want_audio)
            for j in range(passes[i]):
                out_grads += [gr if wneed[wat + 16 * j + k] else None for k, gr in enumerate(grads[j])]
            wat += 16 * passes[i]
            member_audio.append(ga)
        audio: List[Optional[torch.Tensor]] = [None, None]
        for sig in range(2):        # a member's audio gradient goes back through the pools and is added to the one before
            acc = None
            for i in range(n - 1, -1, -1):
                ga = member_audio[i][sig]
                if acc is not None:
                    up_ = torch.empty(geos[i].B, geos[i].T, device=dev, dtype=torch.float32)
                    _call("msd_avgpool_bwd", ptr(acc), ptr(up_), geos[i].T, geos[i].B, geos[i].T)
                    acc = up_ if ga is None else up_.add_(ga)
                else:
                    acc = ga
            audio[sig] = acc
        return (None, None, None, audio[0], audio[1], None, *out_grads)


def _sn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.spectral_norm(m)


class DiscriminatorS(nn.Module):
    """DiscriminatorS of hifigan_models.py:313-339 with the reference's parameter names: real nn.Conv1d modules wrapped by
    torch.nn.utils.weight_norm (convs.N.weight_g / weight_v / bias) or spectral_norm (weight_orig, buffers weight_u /
    weight_v), kernels (15, 41, 41, 41, 41, 41, 5), strides (1, 2, 2, 4, 4, 1, 1), pads k // 2, conv_post 3 taps to one channel.
    channels / groups: narrow models for tests (the first and last conv are dense; a grouped conv needs 4 .. 64 channels per
    group on either side, multiples of 4).  forward(y, y_hat) -> (y_d_r, y_d_g, fmap_r, fmap_g)."""

    def __init__(self, use_spectral_norm: bool = False, channels: Sequence[int] = (128, 128, 256, 512, 1024, 1024, 1024),
                 groups: Sequence[int] = (1, 4, 16, 16, 16, 16, 1)):
        super().__init__()
        ch, gr = tuple(int(c) for c in channels), tuple(int(g) for g in groups)
        if len(ch) != 7 or len(gr) != 7 or any(c <= 0 or c % 4 for c in ch) or gr[0] != 1 or gr[6] != 1:
            raise ValueError(f"DiscriminatorS: seven channels (positive multiples of 4) and seven groups (the first and last 1), "
                             f"got {ch} and {gr}")
        for l in range(1, 6):
            if gr[l] < 1 or ch[l - 1] % gr[l] or ch[l] % gr[l] or any(c // gr[l] % 4 or not 4 <= c // gr[l] <= 64 for c in (ch[l - 1], ch[l])):
                raise ValueError(f"DiscriminatorS: convs.{l} with {ch[l - 1]} -> {ch[l]} channels in {gr[l]} groups: a group needs "
                                 "4 .. 64 channels on either side, multiples of 4")
        self.channels, self.groups, self.use_spectral_norm = ch, gr, bool(use_spectral_norm)
        norm_f = _sn if use_spectral_norm else _wn
        cin, convs = 1, []
        for l, c in enumerate(ch):
            convs.append(norm_f(nn.Conv1d(cin, c, MSD_KERNELS[l], MSD_STRIDES[l], groups=gr[l], padding=MSD_KERNELS[l] // 2)))
            cin = c
        self.convs = nn.ModuleList(convs)
        self.conv_post = norm_f(nn.Conv1d(cin, 1, 3, 1, padding=1))

    def _layers(self):
        return list(self.convs) + [self.conv_post]

    def remove_weight_norm(self):
        for m in self._layers():
            if "weight_g" in m._parameters:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    nn.utils.remove_weight_norm(m)

    def apply_weight_norm(self):
        if self.use_spectral_norm:
            return
        for m in self._layers():
            if "weight_g" not in m._parameters:
                _wn(m)

    def _weights(self) -> List[torch.Tensor]:
        """(weight, bias) of the eight convs, reference layouts, norms folded with torch ops so that autograd carries the
        node's gradient of the folded weight on.  A spectral-norm conv in training mode advances its buffers by one power
        iteration per call, as a call of the reference's module does"""
        out = []
        for m in self._layers():
            if "weight_g" in m._parameters:
                out.append(fold_weight_norm(m.weight_v.float(), m.weight_g.float()))
            elif "weight_orig" in m._parameters:
                out.append(fold_spectral_norm(m.weight_orig, m.weight_u, m.weight_v, self.training))
            else:
                out.append(m.weight)
            out.append(m.bias)
        return out

    def _weight_sets(self) -> List[List[torch.Tensor]]:
        """one set, or two for spectral norm in training mode: the reference calls d(y), then d(y_hat)"""
        return [self._weights() for _ in range(2 if self.use_spectral_norm and self.training else 1)]

    def forward(self, y, y_hat):
        r, g_, fr, fg = _run_s([self], "views", y, y_hat, None)
        return r[0], g_[0], fr[0], fg[0]


@fp32_region
def _run_s(discs: Sequence[DiscriminatorS], mode: str, y, y_hat, len_ratios):
    y2, yh2 = _audio(y, y_hat)
    B, T = y2.shape
    geos, t = [], T
    for d in discs:                                                       # every refusal comes before the first launch
        geos.append(_GeometryS(d.channels, d.groups, B, t))
        t = t // 2 + 1
    for d in discs:
        if any(p_.dtype != torch.float32 for p_ in d.parameters()) or any(b.dtype != torch.float32 for b in d.buffers()):
            raise RadmmmError("MultiScaleDiscriminator is fp32 only")
    cnt = _counts(len_ratios, geos, B, y2.device) if mode != "views" else None
    sets = [d._weight_sets() for d in discs]
    passes = [len(s) for s in sets]
    outs = _MSDFn.apply(mode, geos, passes, y2, yh2, cnt, *[w for s in sets for ws in s for w in ws])
    if mode != "views":
        return outs
    rs, gs, frs, fgs = [], [], [], []
    for i, g in enumerate(geos):
        r, g_, fr, fg = _views_s(g, outs[8 * i:8 * i + 8])
        rs.append(r), gs.append(g_), frs.append(fr), fgs.append(fg)
    return rs, gs, frs, fgs


class MultiScaleDiscriminator(nn.Module):
    """MultiScaleDiscriminator of hifigan_models.py:342-371: members discriminators.0 (spectral norm), .1, .2 on the audio,
    the audio pooled once and twice by AvgPool1d(4, 2, padding=2) (length T // 2 + 1); the state_dict keys are the reference's,
    so the `msd` entry of an upstream checkpoint loads with load_state_dict."""

    def __init__(self, channels: Sequence[int] = (128, 128, 256, 512, 1024, 1024, 1024),
                 groups: Sequence[int] = (1, 4, 16, 16, 16, 16, 1)):
        super().__init__()
        self.discriminators = nn.ModuleList(DiscriminatorS(i == 0, channels, groups) for i in range(3))
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2), nn.AvgPool1d(4, 2, padding=2)])   # (no parameters)

    def remove_weight_norm(self):
        for d in self.discriminators:
            d.remove_weight_norm()

    def apply_weight_norm(self):
        for d in self.discriminators:
            d.apply_weight_norm()

    def forward(self, y, y_hat):
        """y, y_hat [B, 1, T] -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) as the reference nests them: outputs [B, H_post], feature
        maps [B, C, H_l], all strided views of the kernels' buffers.  In training mode the spectral-norm member's buffers
        advance twice and its two signals see different weights, as in the reference"""
        return _run_s(list(self.discriminators), "views", y, y_hat, None)

    def discriminator_loss(self, y, y_hat, len_ratios=None):
        """gan_discriminator_loss(*forward(y, y_hat)[:2], len_ratios) -> (loss, r_losses, g_losses); the per-discriminator
        terms are device tensors [3], nothing is read back"""
        return _run_s(list(self.discriminators), "disc", y, y_hat, len_ratios)

    def generator_losses(self, y, y_hat, len_ratios=None):
        """(gan_feature_loss(fmap_rs, fmap_gs, len_ratios), gan_generator_loss(y_d_gs, len_ratios)[0])"""
        return _run_s(list(self.discriminators), "gen", y, y_hat, len_ratios)


def load_msd(path: str, device="cuda") -> MultiScaleDiscriminator:
    """the `msd` entry of an upstream do_* checkpoint -> MultiScaleDiscriminator on `device`"""
    ckpt = torch.load(path, map_location="cpu")
    if "msd" not in ckpt:
        raise KeyError(f"{path} has no 'msd' entry (keys: {sorted(ckpt)[:8]})")
    msd = MultiScaleDiscriminator()
    msd.load_state_dict(ckpt["msd"])
    return msd.to(device)
