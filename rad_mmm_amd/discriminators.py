"""HiFi-GAN's two discriminator families and the three GAN losses on the GPU, forward and backward (reference
vocoders/hifigan_models.py: DiscriminatorP, MultiPeriodDiscriminator, DiscriminatorS, MultiScaleDiscriminator; loss.py:
gan_feature_loss, gan_discriminator_loss, gan_generator_loss), with ragged batches and no device -> host read.

    mpd = MultiPeriodDiscriminator().cuda()                       # periods 2, 3, 5, 7, 11; the reference's state_dict keys
    msd = MultiScaleDiscriminator().cuda()                        # a spectral-norm member and two weight-norm members on pooled audio
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = mpd(y, y_hat)               # y, y_hat [B, 1, T]; the reference's nesting and shapes
    loss_d, r_losses, g_losses = mpd.discriminator_loss(y, y_hat.detach(), len_ratios)     # the D step
    loss_fm, loss_gen = mpd.generator_losses(y, y_hat, len_ratios)                          # the G step

Per member real and generated audio run in ONE pass as 2B signals.  A feature map lives in a channels-last buffer
[2B * p sequences][pad + H + pad rows][C] with zero rows on either side of every sequence, padded for the conv that reads it
(p = 1 for the multi-scale family).  forward() returns strided views of those buffers: zero copies, ordinary differentiable
tensors.  No atomics: equal inputs give equal bits.  Norms are folded with torch ops, as HiFiGANGenerator's training does,
so autograd carries the folded weight's gradient on to weight_g / weight_v / weight_orig.

The multi-period member (csrc/mpd.hip): pad 2, the 5-tap window of a strided conv is one contiguous stretch of
5 * C floats, so every conv but conv_post is ONE framed radmmm_rowgemm_f32 launch (a_item_stride set, lda = stride * C_in,
K = 5 * C_in) followed by radmmm_mpd_repad (leaky relu into the next padded buffer).  The first conv reads a small frame
matrix that radmmm_mpd_fold_frame cuts from the audio (reflect tail, fold, windows).  The multi-scale member (csrc/msd.hip,
DESIGN 4.23): a 16-column frame matrix and a plain row GEMM, five grouped 41-tap convs (one launch per layer, pad 20), then a
dense 5-tap conv and conv_post, which are the multi-period member's last two layers with p = 1.  A spectral-norm member in
training mode runs two passes of B sequences, one weight set each, into the halves of the same buffers.

Both families are ONE autograd node, _DiscFn.  What differs between them sits on the geometry objects (_Geometry,
_GeometryS): the shapes, how a member's tape is built, its own conv layers' gradients, the spelling of the four loss calls
and, for the multi-scale family, the pooling chain around the members.  The masked reductions run in radmmm_{mpd,msd}_fm_terms
/ _finish (fp64).  The backward is one walk, _walk, over a range of sequences (s0, n): conv_post, then the convs downwards (data
gradient of a dense conv = one row GEMM (b_layout 1) + radmmm_mpd_unframe, the adjoint of the framing in gather form, times
the leaky-relu derivative from the saved output; weight gradient = radmmm_wgrad_f32 over an explicit frame matrix; bias
gradient = radmmm_colsum), then the first conv and the audio.  It stops descending once no weight gradient below the
current layer and no audio gradient is wanted, and it walks the generated half alone, the range (S/2, S/2), when only the
generated audio's gradient is.

Semantics are the reference's: reflect pad on the right by p - T % p at the padded length T (T must exceed it), fold
x[b, 0, h, w] = audio[b, h * p + w], AvgPool1d(4, 2, padding=2) between the multi-scale members, leaky relu of slope 0.1, no
factor 2 in the feature loss.  With len_ratios, item b counts ceil(len_ratios[b] * H_l) rows of a feature map and
ceil(len_ratios[b] * H_post * p) flattened positions of a member's output, the torch expression evaluated on the device in
len_ratios' dtype.  The reference's own mask only broadcasts when some ratio is 1; this module is defined by the formula for
any ratios in [0, 1] (a count is read clamped to its size).  fp32 only: parameters and audio are float32.

MultiPeriodDiscriminator.precision = "h3" (opt-in) keeps all of the above and moves the four wide convs of every
member -- forward, data gradient, weight gradient -- to the f16 matrix cores with three split products: csrc/mpd_h3.hip
writes the fp16 pairs in the passes that form the values, radmmm_rowgemm_h3 reads the padded pair through the same framed
descriptor, radmmm_wgrad_rm contracts a framed pair with the gradient's pair.
"""
from __future__ import annotations

import ctypes
import math
import warnings
from typing import List, Optional, Sequence

import torch
from torch import nn

from . import ops
from ._lib import RadmmmError, check, f32c, fp32_region, lib, ptr, rowgemm, rowgemm_h3, stream
from .vocoder import fold_weight_norm
from .waveglow import _colsum, _wgrad

LRELU_SLOPE = 0.1
MPD_PRECISIONS = ("fp32", "h3")        # MultiPeriodDiscriminator.precision
# precision "h3": an activation enters its fp16 pair times _ACT_SCALE (a pair clamps above 60000 / 64 = 937; the lo halves stay
# normal numbers down to |x| = 2e-3 and the pair's absolute floor is 2^-25 / 64), a weight times ops.W_SCALE
_ACT_SCALE = 64.0
_WGRAD_RM_ROWS = 32                    # radmmm_wgrad_rm contracts at least 32 rows: the producers add zero rows up to it
_OPERAND_BYTES = 2 ** 31 - 2 ** 16     # the row GEMM's operands and the kernels' matrices stay below 2 GiB
MSD_KERNELS = (15, 41, 41, 41, 41, 41, 5)
MSD_STRIDES = (1, 2, 2, 4, 4, 1, 1)
_MSD_PAD = (20, 20, 20, 20, 20, 2, 2)          # of the map conv l WRITES

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


def _gemm_h3(name: str, **kw) -> None:
    _count(name)
    rowgemm_h3(nprod=3, **kw)


def _halves(*shape, dev):
    return torch.empty(*shape, device=dev, dtype=torch.float16), torch.empty(*shape, device=dev, dtype=torch.float16)


def _framed_h3(Xp, S, Hin, Cin, st, Wp, Z, H, C, bias=None) -> dict:
    """_framed on the split pairs: the window of the padded pair Xp (a_item_stride and lda_h count halves), the weights' pair
    Wp [C][5 * Cin]"""
    return dict(Ah=Xp[0], Al=Xp[1], lda_h=st * Cin, a_item_stride=(Hin + 4) * Cin, Bh=Wp[0], Bl=Wp[1], ldb_h=5 * Cin, C=Z, ldc=C,
                M=S * H, N=C, K=5 * Cin, T=H, bias=bias, acc_scale=1.0 / (_ACT_SCALE * ops.W_SCALE))


def _dgrad_h3(dZp, S, H, C, Cin, Tp, dF, g_scale) -> dict:
    """the data gradient's GEMM on pairs: dZp [S * H][C] times the transposed weights' pair Tp [5 * Cin][C]"""
    return dict(Ah=dZp[0], Al=dZp[1], lda_h=C, Bh=Tp[0], Bl=Tp[1], ldb_h=C, C=dF, ldc=5 * Cin, M=S * H, N=5 * Cin, K=C, T=H,
                acc_scale=1.0 / (g_scale * ops.W_SCALE))


def auto_grad_scale(B: int, T: int, period: int) -> float:
    """the automatic gradient scale of one DiscriminatorP in precision "h3": 16 times the smallest power of two at or above
    the number of its outputs B * H_post * p, from host sizes alone.  The adversarial terms are means over (at most) that
    many outputs, so the scaled seed 2 (1 - d) g / n is of order 16 .. 64: twelve octaves of fp16 above it for what the
    convs' gains and a ragged batch's smaller normaliser add, and the pairs' absolute floor 2^-25 nine decimal orders below."""
    p = int(period)
    h = (int(T) + p - 1) // p
    for st in (3, 3, 3, 3, 1):
        h = (h - 1) // st + 1
    return 16.0 * float(2 ** max(0, (max(1, int(B) * h * p) - 1).bit_length()))


def _framed(Xin, S, Hin, Cin, st, W, Z, H, C, bias=None) -> dict:
    """the framed row GEMM of one conv: window h' of sequence s is the 5 * Cin floats at padded row st * h'"""
    return dict(A=Xin, lda=st * Cin, a_item_stride=(Hin + 4) * Cin, B=W, ldb=5 * Cin, C=Z, ldc=C, M=S * H, N=C, K=5 * Cin, T=H,
                bias=bias)


# ---------------------------------------------------------------------------------------------------------------------------
# The members' geometries.  Common attributes: B, T, p (sequences per signal and item), S = 2B * p sequences, s = (sig * B + b)
# * p + w; C, H, stride, pad of the nl convs below conv_post and of the maps they write; K0 / taps0, the first conv's frame
# width and taps; family / lead / terms_tail / grad_tail, the spelling of the four loss calls; wtail, the trailing axes of a
# weight in the reference's layout; period_axis, whether the views keep the axis of length p.  A tape is F1 (the first conv's
# frames), X[0 .. nl - 1] (the padded maps), out [2B, H_post, p] and W, one list of packed weights per pass.
class _Member:
    """what the two families share.  The defaults are the multi-period family's: dense 5-tap convs, every member on the audio
    itself"""

    def n_weights(self) -> int:
        """(weight, bias) of every conv, conv_post included: the node's weight inputs per pass"""
        return 2 * len(self.C) + 2

    def maps(self):
        """(channels, rows) of the maps the losses read, the output last"""
        return self.C + [1], self.H + [self.H[-1]]

    def member_input(self, prev: Optional["_Member"], inp):
        """(y, y_hat, their row stride) of this member from those of the member before it"""
        return inp

    def conv_wgrad(self, l: int, dZ, Xin, n: int):
        """dense 5-tap conv l on n sequences: mpd_frame + the split-K weight gradient + the bias' column sum"""
        C, H, Cin, Hin, R = self.C[l], self.H[l], self.C[l - 1], self.H[l - 1], n * self.H[l]
        Fr = dZ.new_empty(R, 5 * Cin)
        _call("mpd_frame", ptr(Xin), ptr(Fr), n, Hin, Cin, H, self.stride[l])
        _count("wgrad")
        dw = _wgrad(dZ, C, C, Fr, 5 * Cin, 5 * Cin, R, R)[0]
        del Fr
        _count("colsum")
        w = dw.view(C, 5, Cin).permute(0, 2, 1)
        return w.unsqueeze(-1) if self.wtail else w, _colsum(dZ, C, R, C)

    def post_dgrad(self, dOut, W, add, Xin, n: int, need32: bool):
        """conv_post's data gradient on n sequences (+ add, times the leaky-relu derivative) -> dZ of the last conv.  need32:
        is the fp32 array wanted (a weight gradient reads it)?  Only a precision that also keeps a pair asks"""
        dZ = dOut.new_empty(n * self.H[-1], self.C[-1])
        _call("mpd_conv_post_dgrad", ptr(dOut), ptr(W), ptr(add), ptr(Xin), ptr(dZ), n // self.p, self.p, self.H[-1], self.C[-1],
              LRELU_SLOPE)
        return dZ

    def conv_dgrad(self, l: int, dZ, W, add, Xin, n: int, need32: bool = True):
        """dense 5-tap conv l on n sequences: the b_layout-1 GEMM, then mpd_unframe (+ add, times the leaky-relu derivative)"""
        C, H, Cin, Hin, R = self.C[l], self.H[l], self.C[l - 1], self.H[l - 1], n * self.H[l]
        dF = dZ.new_empty(R, 5 * Cin)
        _gemm("dgrad", A=dZ, lda=C, B=W, ldb=5 * Cin, b_layout=1, C=dF, ldc=5 * Cin, M=R, N=5 * Cin, K=C, T=H)
        dX = dZ.new_empty(n * Hin, Cin)
        _call("mpd_unframe", ptr(dF), ptr(add), ptr(Xin), ptr(dX), n, Hin, Cin, H, self.stride[l], LRELU_SLOPE)
        return dX

    def merge_audio(self, geos, member_audio):
        """called after every member with the (dy, dy_hat) pairs not merged yet -> the pairs to carry on, ONE pair after the
        last member.  Here every member sees the audio itself: add the gradients as they come, one running sum per signal"""
        if len(member_audio) == 2:
            acc, ga = member_audio
            member_audio = [[a if b is None else b if a is None else a.add_(b) for a, b in zip(acc, ga)]]
        return member_audio


class _Geometry(_Member):
    """shapes of one DiscriminatorP for B items of T samples"""
    family, K0, taps0, wtail, period_axis = "mpd", 8, 5, (1,), True

    def __init__(self, period: int, channels: Sequence[int], B: int, T: int, h3: Optional[dict] = None):
        """h3: None (fp32), or the state of precision "h3": grad_scale (None: auto_grad_scale), flag (the device int32 [1]
        saturation word), cache / keys (the owner's split weight copies and its parameters' versions per conv).  A plan
        query passes an empty dict"""
        p = self.p = int(period)
        self.h3 = h3
        self.B, self.T = B, T
        n_pad = (p - T % p) % p
        if T <= n_pad:
            raise ValueError(f"DiscriminatorP(period {p}): {T} samples cannot be reflect-padded by {n_pad}")
        self.H0 = (T + n_pad) // p
        self.S = 2 * B * p
        self.C = [int(c) for c in channels]                       # output channels of the five convs
        self.stride, self.pad = [3, 3, 3, 3, 1], [2] * 5
        self.H = []                                               # output rows of the five convs
        h = self.H0
        for st in self.stride:
            h = (h - 1) // st + 1
            self.H.append(h)
        worst = max(self.S * (self.H[l] + 4) * max(self.C[l], 5 * self.C[l - 1] if l else 8) for l in range(5))
        if 4 * worst > _OPERAND_BYTES:
            raise ValueError(f"DiscriminatorP(period {p}): {B} x {T} samples need a GEMM operand of {4 * worst} bytes, above "
                             f"the row GEMM's limit of {_OPERAND_BYTES}: split the batch")
        self.lead = (B, p)
        # per conv (conv_post last) how it runs and why: the ONE decision the launches and precision_plan() share
        if h3 is None:
            self.plan = [("fp32", "precision 'fp32'")] * 6
        else:
            self.plan = [("fp32", "one input channel: an 8-column frame matrix, not a split operand")]
            for l in range(1, 5):
                ok = int(lib.radmmm_mpdh3_plan(self.S, self.H[l - 1], self.C[l - 1], self.H[l], self.C[l], self.stride[l]))
                self.plan.append(("h3", "") if ok == 1 else ("fp32", lib.radmmm_last_error().decode()))
            self.plan.append(("fp32", "one output channel: a wave reduction, not a GEMM"))
            self.g_scale = float(h3["grad_scale"]) if h3.get("grad_scale") is not None else auto_grad_scale(B, T, p)
        self.mode = [m for m, _ in self.plan]
        self.h3w: dict = {}                                       # conv -> (Wh, Wl, Th, Tl) of the pass that ran forward

    def h3_descriptors(self, n: Optional[int] = None) -> List[dict]:
        """every split GEMM descriptor an "h3" step over n sequences (default: all) builds, with the integer 256 for each
        address: what rowgemm_h3_plan is asked in the tests"""
        a, out = 256, []
        n = self.S if n is None else n
        for l in range(1, 5):
            if self.mode[l] != "h3":
                continue
            C, H, Cin, Hin, st = self.C[l], self.H[l], self.C[l - 1], self.H[l - 1], self.stride[l]
            out.append(_framed_h3((a, a), n, Hin, Cin, st, (a, a), a, H, C, a))
            out.append(_dgrad_h3((a, a), n, H, C, Cin, (a, a), a, self.g_scale))
        return out

    def map_sizes(self) -> List[int]:
        """what len_ratios is multiplied with: the rows of the six maps, then the flattened length of the output"""
        return self.H + [self.H[4], self.H[4] * self.p]

    def _split_weights(self, l: int, w: torch.Tensor):
        """the pair of conv l's packed weight [C][5 * Cin] times ops.W_SCALE and of its transpose [5 * Cin][C]: made once per
        parameter version and kept with the owner, so a step after optimizer.step() splits again and two calls without one
        share the copies.  The key is (data_ptr, _version) of the conv's raw parameters, as HiFiGANGenerator._fold's: a write
        that moves neither (through .data or a raw pointer) would leave stale copies; FlatAdam.step advances the version"""
        h3 = self.h3
        key = (h3["keys"][l], w.device)
        ent = h3["cache"].get(l)
        if ent is None or ent[0] != key:
            C, K = self.C[l], 5 * self.C[l - 1]
            Wp = w.detach().float()[..., 0].permute(0, 2, 1).reshape(C, K).contiguous()
            _count("split_w")
            Wh, Wl = ops.split_f16(Wp, K, ops.W_SCALE, K, sat_flag=h3["flag"])
            _count("transpose_w")
            Th, Tl = ops.transpose_split(Wh.view(1, C, K), Wl.view(1, C, K), C, K, C)
            ent = h3["cache"][l] = (key, Wh, Wl, Th[0], Tl[0])
        return ent[1:]

    def terms_tail(self, l: int):
        return (int(l < 5),)                                      # a padded map, or the output

    def grad_tail(self, l: int):
        return ()

    def _pack_weights(self, ws: Sequence[torch.Tensor]):
        """reference layouts (folded) -> GEMM layouts.  convs.0 [C1, 1, 5, 1] -> [C1, 8] (taps, zero padded); convs.l
        [Cout, Cin, 5, 1] -> [Cout, 5 * Cin] with k = tap * Cin + ci; conv_post [1, C, 3, 1] -> [3, C]"""
        out = []
        w0 = ws[0].detach().float()
        W0 = torch.zeros(self.C[0], 8, device=w0.device, dtype=torch.float32)
        W0[:, :5] = w0.reshape(self.C[0], 5)
        out.append(W0)
        for l in range(1, 5):
            # "h3": its pairs instead.  The hi half only fills the tape's slot; the backward takes the four copies from
            # self.h3w, which holds because a geometry is built per call and its node alone keeps it (ctx.geos).  The
            # copies are the owner's cached tensors, never written again: a later version gets new tensors
            if self.mode[l] == "h3":
                self.h3w[l] = self._split_weights(l, ws[2 * l])
                out.append(self.h3w[l][0])
                continue
            out.append(ws[2 * l].detach().float()[..., 0].permute(0, 2, 1).reshape(self.C[l], 5 * self.C[l - 1]).contiguous())
        out.append(ws[10].detach().float().reshape(self.C[4], 3).t().contiguous())
        return out

    def forward(self, y: torch.Tensor, y_hat: torch.Tensor, ldy: int, weight_sets) -> dict:
        """one discriminator on both signals -> its tape (one pass: there is no spectral norm here)"""
        dev, ws = y.device, weight_sets[0]
        S, p, B, T = self.S, self.p, self.B, self.T

        def empty(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)

        W = self._pack_weights(ws)
        bias = [f32c(ws[2 * l + 1].detach()) for l in range(6)]
        F1 = empty(S * self.H[0], 8)
        _call("mpd_fold_frame", ptr(y), ptr(y_hat), ldy, ptr(F1), B, T, p, self.H0, self.H[0])
        X, Xp = [], None                                          # Xp: the pair of the last map, when an "h3" conv reads it
        for l in range(5):
            C, H = self.C[l], self.H[l]
            Z = empty(S * H, C)
            if l == 0:
                _gemm("conv", A=F1, lda=8, B=W[0], ldb=8, C=Z, ldc=C, M=S * H, N=C, K=8, T=H, bias=bias[0])
            elif self.mode[l] == "h3":
                _gemm_h3("conv_h3", **_framed_h3(Xp, S, self.H[l - 1], self.C[l - 1], self.stride[l], self.h3w[l], Z, H, C, bias[l]))
            else:
                Cin, Hin, st = self.C[l - 1], self.H[l - 1], self.stride[l]
                _gemm("conv", **_framed(X[l - 1], S, Hin, Cin, st, W[l], Z, H, C, bias[l]))
            Xl = empty(S, H + 4, C)
            if l < 4 and self.mode[l + 1] == "h3":
                Xp = _halves(S, H + 4, C, dev=dev)
                _call("mpdh3_repad", ptr(Z), C, ptr(Xl), ptr(Xp[0]), ptr(Xp[1]), S, H, C, LRELU_SLOPE, _ACT_SCALE, ptr(self.h3["flag"]))
            else:
                Xp = None
                _call("mpd_repad", ptr(Z), C, ptr(Xl), S, H, C, LRELU_SLOPE)
            X.append(Xl)
        out = empty(2 * B, self.H[4], p)
        _call("mpd_conv_post", ptr(X[4]), ptr(W[5]), ptr(bias[5]), ptr(out), 2 * B, p, self.H[4], self.C[4])
        return {"F1": F1, "X": X, "out": out, "W": [W]}

    def unframe_audio(self, dF, j: int):
        """signal j of the first conv's frame gradients dF -> its audio gradient [B, T]"""
        ga = dF.new_empty(self.B, self.T)
        _call("mpd_unfold_audio", ptr(dF), ptr(ga), self.T, self.B, self.T, self.p, self.H0, self.H[0], j)
        return ga

    # ---- precision "h3": the gradient of an "h3" conv's output is (dZ fp32 or None, dZh, dZl), the pair times g_scale with
    # zero rows up to radmmm_wgrad_rm's minimum; a producer writes it in the pass that forms the gradient
    def _dz_h3(self, l: int, n: int, like, need32: bool):
        R, C = n * self.H[l], self.C[l]
        pair = _halves(max(R, _WGRAD_RM_ROWS), C, dev=like.device)
        return (like.new_empty(R, C) if need32 else None), pair[0], pair[1]

    def post_dgrad(self, dOut, W, add, Xin, n: int, need32: bool):
        if self.mode[4] != "h3":
            return super().post_dgrad(dOut, W, add, Xin, n, need32)
        dZ = self._dz_h3(4, n, dOut, need32)
        _call("mpdh3_conv_post_dgrad", ptr(dOut), ptr(W), ptr(add), ptr(Xin), ptr(dZ[0]), ptr(dZ[1]), ptr(dZ[2]), self.C[4],
              n // self.p, self.p, self.H[4], self.C[4], LRELU_SLOPE, _WGRAD_RM_ROWS, self.g_scale, ptr(self.h3["flag"]))
        return dZ

    def conv_wgrad(self, l: int, dZ, Xin, n: int):
        """an "h3" conv: the windows cut straight into a pair (no fp32 frames), contracted with the dZ pair by radmmm_wgrad_rm
        at one tap over max(R, 32) rows as ONE utterance; the split-K slabs are added in a fixed order"""
        if self.mode[l] != "h3":
            return super().conv_wgrad(l, dZ, Xin, n)
        C, H, Cin, Hin, R = self.C[l], self.H[l], self.C[l - 1], self.H[l - 1], n * self.H[l]
        Rp, K = max(R, _WGRAD_RM_ROWS), 5 * Cin
        Fp = _halves(Rp, K, dev=Xin.device)
        _call("mpdh3_frame", ptr(Xin), ptr(Fp[0]), ptr(Fp[1]), K, n, Hin, Cin, H, self.stride[l], _WGRAD_RM_ROWS, _ACT_SCALE,
              ptr(self.h3["flag"]))
        _count("wgrad_rm")
        P = ops.wgrad_rm_slabs((dZ[1], dZ[2]), Fp, 1, Rp, C, K, 1, 1, 1.0 / (self.g_scale * _ACT_SCALE))
        del Fp
        if P.shape[0] > 1:
            dw = P.new_empty(C * K)
            _call("colsum_final", ptr(P), ptr(dw), P.shape[0], C * K)
        else:
            dw = P
        _count("colsum")
        w = dw.view(C, 5, Cin).permute(0, 2, 1)
        return w.unsqueeze(-1), _colsum(dZ[0], C, R, C)

    def conv_dgrad(self, l: int, dZ, W, add, Xin, n: int, need32: bool = True):
        """an "h3" conv: the dZ pair against the transposed weights' pair, then the unframing -- which writes the pair of the
        conv below when that one is "h3" too"""
        if self.mode[l] != "h3" and self.mode[l - 1] != "h3":
            return super().conv_dgrad(l, dZ, W, add, Xin, n)
        C, H, Cin, Hin, R = self.C[l], self.H[l], self.C[l - 1], self.H[l - 1], n * self.H[l]
        if self.mode[l] != "h3":
            dF = dZ.new_empty(R, 5 * Cin)
            _gemm("dgrad", A=dZ, lda=C, B=W, ldb=5 * Cin, b_layout=1, C=dF, ldc=5 * Cin, M=R, N=5 * Cin, K=C, T=H)
        else:
            dF = Xin.new_empty(R, 5 * Cin)
            _gemm_h3("dgrad_h3", **_dgrad_h3(dZ[1:], n, H, C, Cin, self.h3w[l][2:], dF, self.g_scale))
        if self.mode[l - 1] != "h3":
            dX = dF.new_empty(n * Hin, Cin)
            _call("mpd_unframe", ptr(dF), ptr(add), ptr(Xin), ptr(dX), n, Hin, Cin, H, self.stride[l], LRELU_SLOPE)
            return dX
        dX = self._dz_h3(l - 1, n, dF, need32)
        _call("mpdh3_unframe", ptr(dF), ptr(add), ptr(Xin), ptr(dX[0]), ptr(dX[1]), ptr(dX[2]), Cin, n, Hin, Cin, H, self.stride[l],
              LRELU_SLOPE, _WGRAD_RM_ROWS, self.g_scale, ptr(self.h3["flag"]))
        return dX


class _GeometryS(_Member):
    """shapes of one DiscriminatorS for B items of T samples.  Member i > 0 sees the audio pooled i times"""
    family, K0, taps0, wtail, period_axis = "msd", 16, 15, (), False

    def __init__(self, channels: Sequence[int], groups: Sequence[int], B: int, T: int):
        if T < 1:
            raise ValueError(f"DiscriminatorS: {T} samples are too short")
        self.B, self.T, self.S, self.p = B, T, 2 * B, 1
        self.C, self.G = [int(c) for c in channels], [int(g) for g in groups]
        self.stride, self.pad = list(MSD_STRIDES), list(_MSD_PAD)
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
        self.lead = (B,)

    def map_sizes(self) -> List[int]:
        """what len_ratios is multiplied with: the rows of the eight maps, then the length of the output"""
        return self.H + [self.H[6], self.H[6]]

    def terms_tail(self, l: int):
        return (_MSD_PAD[l] if l < 7 else -1,)                    # the map's pad, or the output

    def grad_tail(self, l: int):
        return (_MSD_PAD[l],)

    def _pack_weights(self, ws: Sequence[torch.Tensor]):
        """reference layouts (folded) -> kernel layouts.  convs.0 [C0, 1, 15] -> [C0, 16]; grouped convs.l [Cout, Cin_g, 41] ->
        [G][Cout_g][41 * Cin_g], kk = tap * Cin_g + ci; convs.6 [C6, C5, 5] -> [C6, 5 * C5]; conv_post [1, C6, 3] -> [3, C6]"""
        w0 = ws[0].detach().float()
        W0 = torch.zeros(self.C[0], 16, device=w0.device, dtype=torch.float32)
        W0[:, :15] = w0.reshape(self.C[0], 15)
        out = [W0]
        for l in range(1, 7):
            out.append(ws[2 * l].detach().float().permute(0, 2, 1).contiguous())
        out.append(ws[14].detach().float().reshape(self.C[6], 3).t().contiguous())
        return out

    def _gconv_dims(self, l: int):
        return (self.H[l - 1], self.H[l], self.G[l], self.C[l - 1] // self.G[l], self.C[l] // self.G[l], MSD_KERNELS[l], MSD_STRIDES[l])

    def member_input(self, prev, inp):
        if prev is None:
            return inp
        pooled = torch.empty(2 * self.B, self.T, device=inp[0].device, dtype=torch.float32)
        _call("msd_avgpool", ptr(inp[0]), ptr(inp[1]), inp[2], ptr(pooled), self.B, prev.T)
        return pooled[:self.B], pooled[self.B:], self.T

    def _forward_pass(self, tape: dict, s0: int, n: int, ws: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """sequences [s0, s0 + n) through the eight convs with one weight set -> the packed weights"""
        dev = tape["out"].device
        T, X, C, H = self.T, tape["X"], self.C, self.H
        W = self._pack_weights(ws)
        bias = [f32c(ws[2 * l + 1].detach()) for l in range(8)]
        Z = torch.empty(n * T, C[0], device=dev, dtype=torch.float32)
        _gemm("conv", A=tape["F1"][s0 * T:], lda=16, B=W[0], ldb=16, C=Z, ldc=C[0], M=n * T, N=C[0], K=16, T=T, bias=bias[0])
        _call("msd_repad", ptr(Z), C[0], ptr(X[0][s0:]), n, T, C[0], _MSD_PAD[0], LRELU_SLOPE)
        for l in range(1, 6):
            _call("msd_gconv_fwd", ptr(X[l - 1][s0:]), ptr(W[l]), ptr(bias[l]), ptr(X[l][s0:]), n, *self._gconv_dims(l), _MSD_PAD[l],
                  LRELU_SLOPE)
        Z = torch.empty(n * H[6], C[6], device=dev, dtype=torch.float32)
        _gemm("conv", **_framed(X[5][s0:], n, H[5], C[5], 1, W[6], Z, H[6], C[6], bias[6]))
        _call("mpd_repad", ptr(Z), C[6], ptr(X[6][s0:]), n, H[6], C[6], LRELU_SLOPE)
        _call("mpd_conv_post", ptr(X[6][s0:]), ptr(W[7]), ptr(bias[7]), ptr(tape["out"][s0:]), n, 1, H[6], C[6])
        return W

    def forward(self, y: torch.Tensor, y_hat: torch.Tensor, ldy: int, weight_sets) -> dict:
        """one member on both signals -> its tape.  One weight set: one pass of 2B; two: the real half with the first, the
        generated half with the second"""
        dev = y.device
        B, S, T = self.B, self.S, self.T
        tape = {"F1": torch.empty(S * T, 16, device=dev, dtype=torch.float32),
                "X": [torch.empty(S, self.H[l] + 2 * _MSD_PAD[l], self.C[l], device=dev, dtype=torch.float32) for l in range(7)],
                "out": torch.empty(S, self.H[6], 1, device=dev, dtype=torch.float32)}
        _call("msd_frame15", ptr(y), ptr(y_hat), ldy, ptr(tape["F1"]), B, T)
        if len(weight_sets) == 1:
            tape["W"] = [self._forward_pass(tape, 0, S, weight_sets[0])]
        else:
            tape["W"] = [self._forward_pass(tape, sig * B, B, weight_sets[sig]) for sig in range(2)]
        return tape

    def conv_wgrad(self, l: int, dZ, Xin, n: int):
        if l == 6:
            return super().conv_wgrad(l, dZ, Xin, n)
        _, Hout, G, cig, _, k, _ = dims = self._gconv_dims(l)
        ns, cols = int(lib.radmmm_msd_gconv_wgrad_splits(n, Hout, G, k)), self.C[l] * k * cig
        P, dw = dZ.new_empty(ns, cols), dZ.new_empty(cols)
        _call("msd_gconv_wgrad", ptr(dZ), ptr(Xin), ptr(P), n, *dims)
        _call("colsum_final", ptr(P), ptr(dw), ns, cols)
        del P
        _count("colsum")
        return dw.view(self.C[l], k, cig).permute(0, 2, 1), _colsum(dZ, self.C[l], n * Hout, self.C[l])

    def conv_dgrad(self, l: int, dZ, W, add, Xin, n: int, need32: bool = True):
        if l == 6:
            return super().conv_dgrad(l, dZ, W, add, Xin, n)
        dims = self._gconv_dims(l)
        dX = dZ.new_empty(n * dims[0], self.C[l - 1])
        _call("msd_gconv_dgrad", ptr(dZ), ptr(W), ptr(add), ptr(Xin), ptr(dX), n, *dims, LRELU_SLOPE)
        return dX

    def unframe_audio(self, dF, j: int):
        ga = dF.new_empty(self.B, self.T)
        _call("msd_unframe15", ptr(dF[j * self.B * self.T:]), ptr(ga), self.T, self.B, self.T)
        return ga

    def merge_audio(self, geos, member_audio):
        """after the last member: its audio gradient goes back through the pools and is added to the one before"""
        if len(member_audio) < len(geos):
            return member_audio
        audio: List[Optional[torch.Tensor]] = [None, None]
        for sig in range(2):
            acc = None
            for g, ga in zip(reversed(geos), reversed(member_audio)):
                if acc is not None:
                    up = torch.empty(g.B, g.T, device=acc.device, dtype=torch.float32)
                    _call("msd_avgpool_bwd", ptr(acc), ptr(up), g.T, g.B, g.T)
                    acc = up if ga[sig] is None else up.add_(ga[sig])
                else:
                    acc = ga[sig]
            audio[sig] = acc
        return [audio]


# ---------------------------------------------------------------------------------------------------------------------------
# The backward walk, shared by the families
def _walk(g: _Member, tape: dict, W, s0: int, n: int, dOut, add, want_w: Sequence[bool], want_audio: Sequence[bool]):
    """sequences [s0, s0 + n) backwards with the weight set W.  dOut: gradient of the output; add[l]: gradient of padded map
    l or None; want_w: per conv; want_audio: per signal of THIS range (all S sequences: both; half of them: one entry).  ->
    (weight and bias gradients in the reference's layouts or None, audio gradients [B, T] per signal of the range)"""
    nl, p, C, H = len(g.C), g.p, g.C, g.H
    X = [x[s0:s0 + n] for x in tape["X"]]
    add = [a[s0:s0 + n] if a is not None else None for a in add]
    dOut = dOut[s0 // p:(s0 + n) // p]
    grads: List[Optional[torch.Tensor]] = [None] * g.n_weights()
    g_audio: List[Optional[torch.Tensor]] = [None] * len(want_audio)

    def below(l):                                   # is anything under conv l still wanted?
        return any(want_w[:l]) or any(want_audio)

    if want_w[nl]:
        cols = 3 * C[-1] + 1
        np_ = int(lib.radmmm_mpd_conv_post_wgrad_parts(n // p, p, H[-1]))
        part, dw = dOut.new_empty(np_, cols), dOut.new_empty(cols)
        _call("mpd_conv_post_wgrad", ptr(dOut), ptr(X[-1]), ptr(part), n // p, p, H[-1], C[-1])
        _call("colsum_final", ptr(part), ptr(dw), np_, cols)
        grads[2 * nl], grads[2 * nl + 1] = dw[:cols - 1].view(3, C[-1]).t().reshape(1, C[-1], 3, *g.wtail), dw[cols - 1:]
    if not below(nl):
        return grads, g_audio
    dZ = g.post_dgrad(dOut, W[nl], add[-1], X[-1], n, want_w[nl - 1])
    for l in range(nl - 1, 0, -1):
        if want_w[l]:
            grads[2 * l], grads[2 * l + 1] = g.conv_wgrad(l, dZ, X[l - 1], n)
        if not below(l):
            return grads, g_audio
        dZ = g.conv_dgrad(l, dZ, W[l], add[l - 1], X[l - 1], n, want_w[l - 1])
    K, R = g.K0, n * H[0]
    if want_w[0]:
        _count("wgrad")
        dw = _wgrad(dZ, C[0], C[0], tape["F1"][s0 * H[0]:], K, K, R, R)[0]
        _count("colsum")
        grads[0], grads[1] = dw[:, :g.taps0].reshape(C[0], 1, g.taps0, *g.wtail), _colsum(dZ, C[0], R, C[0])
    if any(want_audio):
        dF = dZ.new_empty(R, K)
        _gemm("dgrad_audio", A=dZ, lda=C[0], B=W[0], ldb=K, b_layout=1, C=dF, ldc=K, M=R, N=K, K=C[0], T=H[0])
        g_audio = [g.unframe_audio(dF, j) if want else None for j, want in enumerate(want_audio)]
    return grads, g_audio


def _member_backward(g: _Member, tape: dict, dOut, add, want_w, want_audio):
    """want_w: per pass, per conv.  -> (per pass the weight and bias gradients, audio gradients of (y, y_hat))"""
    S = g.S
    if len(tape["W"]) == 1:
        if not any(want_w[0]) and not want_audio[0]:
            if not want_audio[1]:
                return [[None] * g.n_weights()], [None, None]
            # only the generated signal's audio gradient is wanted: walk its half of every buffer alone
            gr, ga = _walk(g, tape, tape["W"][0], S // 2, S // 2, dOut, add, want_w[0], [True])
            return [gr], [None, ga[0]]
        gr, ga = _walk(g, tape, tape["W"][0], 0, S, dOut, add, want_w[0], want_audio)
        return [gr], ga
    grads, audio = [], []
    for sig in range(2):                            # two weight sets: each signal's half with its own
        if any(want_w[sig]) or want_audio[sig]:
            gr, ga = _walk(g, tape, tape["W"][sig], sig * S // 2, S // 2, dOut, add, want_w[sig], [want_audio[sig]])
        else:
            gr, ga = [None] * g.n_weights(), [None]
        grads.append(gr)
        audio.append(ga[0])
    return grads, audio


def _views(g: _Member, bufs: Sequence[torch.Tensor]):
    """the buffers of one member (its padded maps, then the output) -> (y_d_r, y_d_g, fmap_r, fmap_g): strided views, no
    copies; [.., H, p] for the multi-period family, [.., H] for the multi-scale one"""
    B, p, nl = g.B, g.p, len(g.C)
    shape = (lambda v: v) if g.period_axis else (lambda v: v.squeeze(-1))
    fm = ([], [])
    for l in range(nl):
        pad, H = g.pad[l], g.H[l]
        v = shape(bufs[l].view(2, B, p, H + 2 * pad, g.C[l])[:, :, :, pad:pad + H, :].permute(0, 1, 4, 3, 2))   # [2, B, C, H, p]
        fm[0].append(v[0])
        fm[1].append(v[1])
    out = shape(bufs[nl].view(2, B, 1, g.H[-1], p))
    fm[0].append(out[0])
    fm[1].append(out[1])
    return out[0].reshape(B, g.H[-1] * p), out[1].reshape(B, g.H[-1] * p), fm[0], fm[1]


class _DiscFn(torch.autograd.Function):
    """The members of one family as one autograd node.  Inputs: mode, the geometries, passes (weight sets per member: 1, or 2
    for a spectral-norm member in training mode), y [B, T], y_hat [B, T], cnt (int32 [members, maps + 1, B] or None), then per
    member and pass (weight, bias) of its convs, reference layouts, norms already folded.  mode "views": the outputs are the
    buffers forward() cuts its views from (per member the padded maps and the output).  mode "disc": (loss, r_losses [n],
    g_losses [n]).  mode "gen": (loss_fm, loss_gen)."""

    @staticmethod
    def forward(ctx, mode, geos, passes, y, y_hat, cnt, *weights):
        dev = y.device
        y, y_hat = f32c(y.detach()), f32c(y_hat.detach())
        n = len(geos)
        tapes, at, inp = [], 0, (y, y_hat, y.shape[1])
        for i, g in enumerate(geos):
            inp = g.member_input(geos[i - 1] if i else None, inp)
            nw = g.n_weights()
            tapes.append(g.forward(*inp, [weights[at + nw * j:at + nw * (j + 1)] for j in range(passes[i])]))
            at += nw * passes[i]
        ctx.mode, ctx.geos, ctx.passes, ctx.has_cnt = mode, geos, passes, cnt is not None
        ctx.set_materialize_grads(False)
        keep = [b for t in tapes for b in (t["F1"], *t["X"], t["out"], *[w for W in t["W"] for w in W])]
        if mode == "views":
            ctx.save_for_backward(*keep)
            return tuple(b for t in tapes for b in (*t["X"], t["out"]))
        res = torch.empty(n, 4, device=dev, dtype=torch.float32)
        norm = torch.empty(n, len(geos[0].C) + 3, device=dev, dtype=torch.float64)
        i32 = ctypes.c_int32
        for i, (g, t) in enumerate(zip(geos, tapes)):
            ci = cnt[i] if cnt is not None else None
            with_fm = mode == "gen"
            Cs, Hs = g.maps()
            nm = len(Cs)
            offs = [0]
            for l in range(nm):
                offs.append(offs[-1] + (int(lib.radmmm_mpd_fm_terms_parts(g.B, g.p, Hs[l], Cs[l])) if with_fm else 0))
            part = torch.empty(max(offs[-1], 1), device=dev, dtype=torch.float32)
            if with_fm:
                for l in range(nm):
                    src = t["X"][l] if l < nm - 1 else t["out"]
                    _call(g.family + "_fm_terms", ptr(src), ptr(ci[l]) if ci is not None else None, ptr(part[offs[l]:]), *g.lead,
                          Hs[l], Cs[l], *g.terms_tail(l))
            _call(g.family + "_finish", ptr(part), (i32 * (nm + 1))(*offs), (i32 * nm)(*Cs), (i32 * nm)(*Hs), ptr(t["out"]), ptr(ci),
                  ptr(res[i]), ptr(norm[i]), *g.lead)
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
        for g, np_ in zip(geos, passes):            # per member: F1, the maps, out, then the packed weights of every pass
            nl = len(g.C)
            w_at = at + nl + 2
            tapes.append({"F1": saved[at], "X": saved[at + 1:at + 1 + nl], "out": saved[at + 1 + nl],
                          "W": [saved[w_at + (nl + 1) * j:w_at + (nl + 1) * (j + 1)] for j in range(np_)]})
            at = w_at + (nl + 1) * np_
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
        wat = oat = 0
        for i, (g, t) in enumerate(zip(geos, tapes)):
            nl, nw = len(g.C), g.n_weights()
            want_w = [[bool(wneed[wat + nw * j + 2 * l] or wneed[wat + nw * j + 2 * l + 1]) for l in range(nl + 1)]
                      for j in range(passes[i])]
            if mode == "views":
                gb = gouts[oat:oat + nl + 1]
                oat += nl + 1
                add = [f32c(x) if x is not None else None for x in gb[:nl]]
                dOut = f32c(gb[nl]) if gb[nl] is not None else torch.zeros_like(t["out"])
            else:
                ci = cnt[i] if cnt is not None else None
                add = [None] * nl
                if mode == "gen":
                    for l in range(nl):
                        add[l] = torch.empty_like(t["X"][l])
                        _call(g.family + "_fm_grad", ptr(t["X"][l]), ptr(ci[l]) if ci is not None else None, ptr(norm[i, l:]),
                              ptr(up[i]), ptr(add[l]), *g.lead, g.H[l], g.C[l], *g.grad_tail(l))
                dOut = torch.empty_like(t["out"])
                _call(g.family + "_out_grad", ptr(t["out"]), ptr(ci), ptr(norm[i]), ptr(up[i]), ptr(dOut), *g.lead, g.H[-1])
            grads, ga = _member_backward(g, t, dOut, add, want_w, want_audio)
            for j in range(passes[i]):
                out_grads += [gr if wneed[wat + nw * j + k] else None for k, gr in enumerate(grads[j])]
            wat += nw * passes[i]
            member_audio = g.merge_audio(geos, member_audio + [ga])      # merges what the family can merge by now
        audio = member_audio[0]                                          # after the last member: one (y, y_hat) pair
        return (None, None, None, audio[0], audio[1], None, *out_grads)


def _audio(y: torch.Tensor, y_hat: torch.Tensor):
    if not (isinstance(y, torch.Tensor) and isinstance(y_hat, torch.Tensor) and y.is_cuda and y_hat.is_cuda):
        raise RadmmmError("MultiPeriodDiscriminator needs GPU tensors (there is no CPU path)")
    if y.shape != y_hat.shape or y.dim() != 3 or y.shape[1] != 1:
        raise ValueError(f"MultiPeriodDiscriminator: y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must both be [B, 1, T]")
    return y.reshape(y.shape[0], y.shape[2]), y_hat.reshape(y.shape[0], y.shape[2])


def _counts(len_ratios, geos: Sequence[_Member], B: int, dev: torch.device) -> Optional[torch.Tensor]:
    """the reference's (len_ratios * size).ceil().long() for every size in map_sizes() of every member, in len_ratios' dtype
    on the device, as int32 [members, sizes, B]: 7 sizes for the multi-period, 9 for the multi-scale discriminator (the
    kernels read it clamped to [0, size])"""
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
def _run(discs: Sequence["_Discriminator"], mode: str, y, y_hat, len_ratios, h3: Optional[dict] = None):
    y2, yh2 = _audio(y, y_hat)
    B, T = y2.shape
    # every refusal comes before the first launch
    geos = discs[0]._geometries(discs, B, T) if h3 is None else discs[0]._geometries(discs, B, T, h3)
    for d in discs:
        if any(t.dtype != torch.float32 for t in (*d.parameters(), *d.buffers())):
            raise RadmmmError(f"{d._multi} is fp32 only")
    cnt = _counts(len_ratios, geos, B, y2.device) if mode != "views" else None
    sets = [d._weight_sets() for d in discs]
    outs = _DiscFn.apply(mode, geos, [len(s) for s in sets], y2, yh2, cnt, *[w for s in sets for ws in s for w in ws])
    if mode != "views":
        return outs
    rs, gs, frs, fgs, at = [], [], [], [], 0
    for g in geos:
        r, g_, fr, fg = _views(g, outs[at:at + len(g.C) + 1])
        at += len(g.C) + 1
        rs.append(r), gs.append(g_), frs.append(fr), fgs.append(fg)
    return rs, gs, frs, fgs


def _wn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.weight_norm(m)


def _sn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.spectral_norm(m)


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


class _Discriminator(nn.Module):
    """one member: self.convs, self.conv_post, self.use_spectral_norm; forward(y, y_hat) -> (y_d_r, y_d_g, fmap_r, fmap_g)"""

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
        """(weight, bias) of every conv, reference layouts, norms folded with torch ops so that autograd carries the node's
        gradient of the folded weight on.  A spectral-norm conv in training mode advances its buffers by one power iteration
        per call, as a call of the reference's module does"""
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
        r, g_, fr, fg = _run([self], "views", y, y_hat, None)
        return r[0], g_[0], fr[0], fg[0]


class _MultiDiscriminator(nn.Module):
    """self.discriminators: the members of one family"""

    def remove_weight_norm(self):
        for d in self.discriminators:
            d.remove_weight_norm()

    def apply_weight_norm(self):
        for d in self.discriminators:
            d.apply_weight_norm()

    def forward(self, y, y_hat):
        """y, y_hat [B, 1, T] -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) as the reference nests them: outputs [B, H_post * p],
        feature maps [B, C, H_l, p] (multi-scale: [B, H_post] and [B, C, H_l]), all strided views of the kernels' buffers.
        In training mode a spectral-norm member's buffers advance twice and its two signals see different weights, as in
        the reference"""
        return _run(list(self.discriminators), "views", y, y_hat, None)

    def discriminator_loss(self, y, y_hat, len_ratios=None):
        """gan_discriminator_loss(*forward(y, y_hat)[:2], len_ratios) -> (loss, r_losses, g_losses); the per-discriminator
        terms are device tensors [n], nothing is read back"""
        return _run(list(self.discriminators), "disc", y, y_hat, len_ratios)

    def generator_losses(self, y, y_hat, len_ratios=None):
        """(gan_feature_loss(fmap_rs, fmap_gs, len_ratios), gan_generator_loss(y_d_gs, len_ratios)[0])"""
        return _run(list(self.discriminators), "gen", y, y_hat, len_ratios)


class DiscriminatorP(_Discriminator):
    """DiscriminatorP(period) of hifigan_models.py:249-283 with the reference's parameter names: convs.N.weight_g / weight_v
    [Cout, Cin, 5, 1] / bias, conv_post.* with a (3, 1) kernel, weight norm over dim 0.  channels: the five convs' widths
    (multiples of 4; narrow models for tests).  forward(y, y_hat) -> (y_d_r, y_d_g, fmap_r, fmap_g)."""
    _multi, use_spectral_norm = "MultiPeriodDiscriminator", False

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
        self._h3_cache: dict = {}                   # precision "h3": conv -> (parameter versions, the weight's split copies)

    @staticmethod
    def _geometries(discs, B: int, T: int, h3: Optional[dict] = None):
        """h3: None, or what MultiPeriodDiscriminator hands down for precision "h3" (grad_scale, flag); every member adds its
        own cache of split weights and the versions of its convs' parameters"""
        if h3 is None:
            return [_Geometry(d.period, d.channels, B, T) for d in discs]
        return [_Geometry(d.period, d.channels, B, T,
                          dict(h3, cache=d._h3_cache, keys=[tuple((p.data_ptr(), p._version) for p in m.parameters()) for m in d.convs]))
                for d in discs]


def _check_precision(name) -> str:
    if name not in MPD_PRECISIONS:
        raise ValueError(f"MultiPeriodDiscriminator: precision {name!r} is none of {MPD_PRECISIONS}")
    return name


class MultiPeriodDiscriminator(_MultiDiscriminator):
    """MultiPeriodDiscriminator of hifigan_models.py:286-310; state_dict keys discriminators.N.convs.M.{weight_g, weight_v,
    bias} and discriminators.N.conv_post.*, so the `mpd` entry of an upstream checkpoint loads with load_state_dict.

    precision: "fp32" (default) or "h3"; forward, discriminator_loss and generator_losses take a per-call precision= that
    overrides it, and any other name raises ValueError before any device work.  In "h3" convs.1 .. convs.4 of every member
    run forward, data gradient and weight gradient on the f16 matrix cores with three split products (radmmm_rowgemm_h3,
    radmmm_wgrad_rm; fp32-class accuracy): the leaky-relu pass writes the next conv's framed fp16 pair beside the fp32 map,
    the backward's unframing writes the gradient's pair, the weight gradient's windows are cut straight into a pair, and the
    weights' split copies are kept per parameter version.  convs.0, conv_post, the norm folds, the bias sums, the loss
    reductions and every feature map stay fp32; a conv the split kernels refuse runs its fp32 path in all three passes
    (precision_plan() says which and why).  Training, eval mode and no_grad all use the mode.  Gradients enter the pairs times
    grad_scale -- None: auto_grad_scale(B, T, period) per member, from host sizes; or a power of two -- and .grad and the
    audio gradient hold the true values.  A pair that clamps at fp16's range (a gradient or a forward activation) raises
    saturation_flag(), the device word that `FlatAdam.step(skip=...)` takes; grad_saturated() reads and clears it, and
    nothing else waits for the device.  A checkpoint does not store the mode."""

    def __init__(self, periods: Sequence[int] = (2, 3, 5, 7, 11), channels: Sequence[int] = (32, 128, 512, 1024, 1024)):
        super().__init__()
        self.discriminators = nn.ModuleList(DiscriminatorP(p, channels) for p in periods)
        self.precision = "fp32"
        self.grad_scale = None                      # precision "h3": None (auto_grad_scale per member) or a power of two
        self._sat_flag = None                       # device int32 [1]: OR-ed by the pair producers of an "h3" call

    def _h3(self, precision) -> Optional[dict]:
        """what a call in `precision` (None: the attribute) hands to the geometries; None for "fp32\""""
        if _check_precision(self.precision if precision is None else precision) == "fp32":
            return None
        g = self.grad_scale
        if g is not None:
            g = float(g)
            if not (g > 0 and g < float("inf") and 2.0 ** round(math.log2(g)) == g):
                raise ValueError(f"grad_scale {self.grad_scale!r} (precision 'h3'): None or a power of two")
        return {"grad_scale": g, "flag": self.saturation_flag()}

    def saturation_flag(self) -> torch.Tensor:
        """the device int32 [1] word a clamped pair of an "h3" call raises (created zeroed), for a guard that stays on the
        device: `FlatAdam.step(skip=mpd.saturation_flag())`.  Clearing it stays with grad_saturated()."""
        dev = next(self.parameters()).device
        if self._sat_flag is None or self._sat_flag.device != dev:
            self._sat_flag = torch.zeros(1, device=dev, dtype=torch.int32)
        return self._sat_flag

    def grad_saturated(self) -> bool:
        """True when a pair of an "h3" call clamped since the last call of this method: reads the device and clears the
        word.  The step's gradients are then not to be used; lower grad_scale (or find the activation that left fp16's range)."""
        if self._sat_flag is None:
            return False
        hit = bool(int(self._sat_flag.item()) & 1)
        self._sat_flag.zero_()
        return hit

    def precision_plan(self, precision: Optional[str] = None, B: Optional[int] = None, T: Optional[int] = None) -> list:
        """per member a dict conv name -> (mode, reason) for a batch of B x T samples (default 1 x 8192): ("h3", "") where the
        three passes reach the split kernels, else ("fp32", why).  Host only: the launches take the same decision from the
        same function (radmmm_mpdh3_plan, which asks radmmm_rowgemm_h3's own planner)."""
        name = _check_precision(self.precision if precision is None else precision)
        B, T = (1 if B is None else int(B)), (8192 if T is None else int(T))
        names = [f"convs.{l}" for l in range(5)] + ["conv_post"]
        return [dict(zip(names, _Geometry(d.period, d.channels, B, T, None if name == "fp32" else {}).plan))
                for d in self.discriminators]

    def forward(self, y, y_hat, precision: Optional[str] = None):
        return _run(list(self.discriminators), "views", y, y_hat, None, self._h3(precision))

    def discriminator_loss(self, y, y_hat, len_ratios=None, precision: Optional[str] = None):
        return _run(list(self.discriminators), "disc", y, y_hat, len_ratios, self._h3(precision))

    def generator_losses(self, y, y_hat, len_ratios=None, precision: Optional[str] = None):
        return _run(list(self.discriminators), "gen", y, y_hat, len_ratios, self._h3(precision))

    forward.__doc__ = _MultiDiscriminator.forward.__doc__
    discriminator_loss.__doc__ = _MultiDiscriminator.discriminator_loss.__doc__
    generator_losses.__doc__ = _MultiDiscriminator.generator_losses.__doc__


def load_mpd(path: str, device="cuda", precision: str = "fp32", **model_kwargs) -> MultiPeriodDiscriminator:
    """the `mpd` entry of an upstream do_* checkpoint -> MultiPeriodDiscriminator on `device`; model_kwargs go to the
    constructor (a checkpoint of a narrow model).  precision: the model's mode (the file does not store one); a bad name
    raises before the file is looked at"""
    _check_precision(precision)
    ckpt = torch.load(path, map_location="cpu")
    if "mpd" not in ckpt:
        raise KeyError(f"{path} has no 'mpd' entry (keys: {sorted(ckpt)[:8]})")
    mpd = MultiPeriodDiscriminator(**model_kwargs)
    mpd.load_state_dict(ckpt["mpd"])
    mpd.precision = precision
    return mpd.to(device)


class DiscriminatorS(_Discriminator):
    """DiscriminatorS of hifigan_models.py:313-339 with the reference's parameter names: real nn.Conv1d modules wrapped by
    torch.nn.utils.weight_norm (convs.N.weight_g / weight_v / bias) or spectral_norm (weight_orig, buffers weight_u /
    weight_v), kernels (15, 41, 41, 41, 41, 41, 5), strides (1, 2, 2, 4, 4, 1, 1), pads k // 2, conv_post 3 taps to one channel.
    channels / groups: narrow models for tests (the first and last conv are dense; a grouped conv needs 4 .. 64 channels per
    group on either side, multiples of 4).  forward(y, y_hat) -> (y_d_r, y_d_g, fmap_r, fmap_g)."""
    _multi = "MultiScaleDiscriminator"

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

    @staticmethod
    def _geometries(discs, B: int, T: int):
        geos = []
        for d in discs:                             # AvgPool1d(4, 2, padding=2) between the members: T -> T // 2 + 1
            geos.append(_GeometryS(d.channels, d.groups, B, T))
            T = T // 2 + 1
        return geos


class MultiScaleDiscriminator(_MultiDiscriminator):
    """MultiScaleDiscriminator of hifigan_models.py:342-371: members discriminators.0 (spectral norm), .1, .2 on the audio,
    the audio pooled once and twice by AvgPool1d(4, 2, padding=2) (length T // 2 + 1); the state_dict keys are the reference's,
    so the `msd` entry of an upstream checkpoint loads with load_state_dict."""

    def __init__(self, channels: Sequence[int] = (128, 128, 256, 512, 1024, 1024, 1024),
                 groups: Sequence[int] = (1, 4, 16, 16, 16, 16, 1)):
        super().__init__()
        self.discriminators = nn.ModuleList(DiscriminatorS(i == 0, channels, groups) for i in range(3))
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2), nn.AvgPool1d(4, 2, padding=2)])   # (no parameters)


def load_msd(path: str, device="cuda", **model_kwargs) -> MultiScaleDiscriminator:
    """the `msd` entry of an upstream do_* checkpoint -> MultiScaleDiscriminator on `device`; model_kwargs go to the
    constructor (a checkpoint of a narrow model)"""
    ckpt = torch.load(path, map_location="cpu")
    if "msd" not in ckpt:
        raise KeyError(f"{path} has no 'msd' entry (keys: {sorted(ckpt)[:8]})")
    msd = MultiScaleDiscriminator(**model_kwargs)
    msd.load_state_dict(ckpt["msd"])
    return msd.to(device)
