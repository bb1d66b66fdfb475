"""Differentiable log-mel and the mel-spectrogram L1 loss on the GPU, forward and backward, with ragged batches and no
device -> host read: the term HiFi-GAN's generator objective weights 45 to 1, computed with THIS project's mel transform
(audio_processing.TacotronSTFT: its window, basis and padding) instead of torch.stft.

    mel = mel_spectrogram(y, stft, lens=None)                 # [B, n_mel, 1 + S // hop] with a grad_fn
    mel_loss = MelSpectrogramLoss().cuda()                    # TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0)
    loss = mel_loss(x, target, lens=None, frames=None)        # 0-d fp32; target: a mel [B, n_mel, Ft] or audio [B, S]

Semantics (reference audio_processing.py TacotronSTFT.mel_spectrogram :137-154 and STFT.transform :227-255, applied to each
item alone at x[b, :lens[b]]): reflect pad by n_fft / 2 about 0 and about lens[b] - 1, 1 + lens[b] // hop frames,
mag = sqrt(re^2 + im^2) without a clamp, mel = log(max(mel_basis @ mag, 1e-5)); loss = F.l1_loss over the frames
f < n[b] = min(1 + lens[b] // hop, Ft, frames[b]).  Subgradients: the clamp passes where melp >= 1e-5 (torch.clamp),
sign(0) = 0, and the gradient of sqrt at re = im = 0 is 0 (torch gives NaN there).

Launches (csrc/mel_loss.hip): radmmm_melloss_frame, row GEMM with forward_basis, radmmm_melloss_mag, row GEMM
with mel_basis, radmmm_melloss_terms, radmmm_melloss_finish forward; radmmm_melloss_bwd, row GEMM, radmmm_melloss_dspec,
row GEMM, radmmm_melloss_unframe backward.  The sign of mel - target is not stored: the backward recomputes it from the
saved melp and the target with the forward's own expression.  fp32 throughout, no atomics: equal calls give equal bits.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import ops
from ._lib import RadmmmError, check, f32c, fp32_region, lib, ptr, rowgemm, stream
from .audio_processing import TacotronSTFT

_OPERAND_BYTES = 2 ** 31 - 2 ** 16     # the row GEMM's operands (and the kernels' matrices here) stay below 2 GiB
_CLIP = 1e-5                           # dynamic_range_compression's clip_val


class _Geometry:
    """shapes of one call: B items of S samples through `stft`; every refusal comes before the first launch"""

    def __init__(self, stft: TacotronSTFT, B: int, S: int, signals: int = 1):
        s = stft.stft_fn
        self.n_fft, self.hop, self.n_mel = int(s.filter_length), int(s.hop_length), int(stft.n_mel_channels)
        if self.n_fft < 4 or self.n_fft % 4 or self.hop < 1:
            raise ValueError(f"mel_loss: needs filter_length % 4 == 0 and hop_length >= 1 (got {self.n_fft}, {self.hop})")
        self.h, self.cutoff = self.n_fft // 2, self.n_fft // 2 + 1
        self.lds, self.ldm, self.ldn = ops.round_up(2 * self.cutoff, 4), ops.round_up(self.cutoff, 4), ops.round_up(self.n_mel, 4)
        if B < 1 or S <= self.h:
            raise ValueError(f"mel_loss: {S} samples cannot be reflect-padded by {self.h} (filter_length {self.n_fft} needs more "
                             f"than {self.h})")
        self.B, self.S, self.F = B, S, 1 + S // self.hop
        self.rows = B * self.F
        if signals * self.rows * max(self.n_fft, self.lds) * 4 >= _OPERAND_BYTES:
            raise ValueError(f"mel_loss: {signals} x {B} x {S} samples at filter_length {self.n_fft}, hop {self.hop} exceed the "
                             "row GEMM's 2 GiB operand limit: split the batch")


def _bases(stft: TacotronSTFT, g: _Geometry, dev: torch.device):
    """(forward_basis [2 cutoff, n_fft], mel_basis zero-padded to [ldn, ldm]) on `dev` in fp32.  The padded copy is kept on
    the module and rebuilt when mel_basis was written to (load_state_dict) or moved."""
    fb, mb = stft.stft_fn.forward_basis, stft.mel_basis
    if not (fb.is_cuda and mb.is_cuda):
        raise RadmmmError("mel_loss: move the TacotronSTFT to the GPU first (there is no CPU path)")
    if tuple(fb.shape) != (2 * g.cutoff, g.n_fft) or tuple(mb.shape) != (g.n_mel, g.cutoff):
        raise ValueError(f"mel_loss: forward_basis {tuple(fb.shape)} / mel_basis {tuple(mb.shape)} do not fit filter_length "
                         f"{g.n_fft} and {g.n_mel} mels")
    key = (mb.data_ptr(), mb._version, mb.device, mb.dtype)
    cache = stft.__dict__.get("_melloss_basis")
    if cache is None or cache[0] != key:
        pad = torch.zeros(g.ldn, g.ldm, device=dev, dtype=torch.float32)
        pad[:g.n_mel, :g.cutoff] = mb.detach()
        cache = (key, pad)
        stft.__dict__["_melloss_basis"] = cache
    return f32c(fb.detach()), cache[1]


def _forward_chain(g: _Geometry, sigs, lens, lens_k, fb, mb):
    """signals [B, S] each -> (spec [k*rows, lds], melp [k*rows, ldn]) of the k stacked signals"""
    k, dev, s = len(sigs), sigs[0].device, stream()
    rows = k * g.rows
    A = torch.empty(rows, g.n_fft, device=dev, dtype=torch.float32)
    for j, sig in enumerate(sigs):
        check(lib.radmmm_melloss_frame(ptr(sig), g.S, ptr(lens), ptr(A[j * g.rows:]), g.B, g.S, g.F, g.n_fft, g.hop, s),
              "melloss_frame")
    spec = torch.empty(rows, g.lds, device=dev, dtype=torch.float32)
    rowgemm(A=A, lda=g.n_fft, B=fb, ldb=g.n_fft, b_tap_stride=0, C=spec, ldc=g.lds, M=rows, N=2 * g.cutoff, K=g.n_fft, T=g.F)
    mag = torch.empty(rows, g.ldm, device=dev, dtype=torch.float32)
    check(lib.radmmm_melloss_mag(ptr(spec), g.lds, ptr(lens_k), ptr(mag), g.ldm, k * g.B, g.S, g.F, g.hop, g.cutoff, s),
          "melloss_mag")
    melp = torch.empty(rows, g.ldn, device=dev, dtype=torch.float32)
    # K runs over the zero pad columns of mag and of the padded mel_basis: cutoff is odd
    rowgemm(A=mag, lda=g.ldm, B=mb, ldb=g.ldm, b_tap_stride=0, C=melp, ldc=g.ldn, M=rows, N=g.ldn, K=g.ldm, T=g.F)
    return spec, melp


def _backward_chain(g: _Geometry, dmelp, spec, lens_k, fb, mb):
    """dmelp [k*rows, ldn] -> dA [k*rows, n_fft]"""
    rows, dev, s = dmelp.shape[0], dmelp.device, stream()
    dmag = torch.empty(rows, g.ldm, device=dev, dtype=torch.float32)
    rowgemm(A=dmelp, lda=g.ldn, B=mb, ldb=g.ldm, b_tap_stride=0, b_layout=1, C=dmag, ldc=g.ldm, M=rows, N=g.ldm, K=g.ldn, T=g.F)
    dspec = torch.empty(rows, g.lds, device=dev, dtype=torch.float32)
    check(lib.radmmm_melloss_dspec(ptr(dmag), g.ldm, ptr(spec), g.lds, ptr(lens_k), ptr(dspec), rows // g.F, g.S, g.F, g.hop,
                                   g.cutoff, s), "melloss_dspec")
    dA = torch.empty(rows, g.n_fft, device=dev, dtype=torch.float32)
    rowgemm(A=dspec, lda=g.lds, B=fb, ldb=g.n_fft, b_tap_stride=0, b_layout=1, C=dA, ldc=g.n_fft, M=rows, N=g.n_fft,
            K=2 * g.cutoff, T=g.F)
    return dA


def _unframe(g: _Geometry, dA, lens):
    dx = torch.empty(g.B, g.S, device=dA.device, dtype=torch.float32)
    check(lib.radmmm_melloss_unframe(ptr(dA), ptr(lens), ptr(dx), g.S, g.B, g.S, g.F, g.n_fft, g.hop, 0, stream()),
          "melloss_unframe")
    return dx


class _MelFn(torch.autograd.Function):
    """(y [B, S], lens int32 [B] or None, stft) -> log-mel [B, n_mel, F] as one autograd node; saves spec and melp"""

    @staticmethod
    def forward(ctx, y, lens, stft):
        g = _Geometry(stft, *y.shape)
        fb, mb = _bases(stft, g, y.device)
        y = f32c(y.detach())
        spec, melp = _forward_chain(g, [y], lens, lens, fb, mb)
        mel = torch.empty(g.B, g.n_mel, g.F, device=y.device, dtype=torch.float32)
        check(lib.radmmm_melloss_terms(ptr(melp), g.ldn, ptr(lens), None, None, 0, ptr(mel), None, g.B, g.S, g.F, g.hop, g.n_mel,
                                       _CLIP, stream()), "melloss_terms")
        ctx.g, ctx.has_lens, ctx.bases = g, lens is not None, (fb, mb)
        ctx.save_for_backward(spec, melp, *([lens] if lens is not None else []))
        return mel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmel):
        spec, melp, *rest = ctx.saved_tensors
        lens = rest[0] if ctx.has_lens else None
        g = ctx.g
        dmel = f32c(dmel)
        dmelp = torch.empty(g.rows, g.ldn, device=dmel.device, dtype=torch.float32)
        check(lib.radmmm_melloss_bwd(ptr(melp), g.ldn, ptr(lens), None, None, 0, None, None, ptr(dmel), ptr(dmelp), g.B, g.S, g.F,
                                     g.hop, g.n_mel, _CLIP, stream()), "melloss_bwd")
        return _unframe(g, _backward_chain(g, dmelp, spec, lens, *ctx.bases), lens), None, None


class _MelLossFn(torch.autograd.Function):
    """(x [B, S], target: mel [B, n_mel, Ft] or audio [B, S], lens, frames, stft, target_is_audio) -> the 0-d loss as one
    autograd node.  Saves the spectra and melp of the signals it transformed, the target mel, the normaliser and, when an
    audio target asks for a gradient, the mel of x."""

    @staticmethod
    def forward(ctx, x, target, lens, frames, stft, target_is_audio):
        want_t = bool(target_is_audio and ctx.needs_input_grad[1])
        g = _Geometry(stft, *x.shape, signals=2 if target_is_audio else 1)
        dev, s = x.device, stream()
        fb, mb = _bases(stft, g, dev)
        x, target = f32c(x.detach()), f32c(target.detach())
        f32 = dict(device=dev, dtype=torch.float32)
        xmel = None
        if target_is_audio:
            lens_k = lens.repeat(2) if lens is not None else None
            spec, melp = _forward_chain(g, [x, target], lens, lens_k, fb, mb)
            tmel, Ft = torch.empty(g.B, g.n_mel, g.F, **f32), g.F
            check(lib.radmmm_melloss_terms(ptr(melp[g.rows:]), g.ldn, ptr(lens), None, None, 0, ptr(tmel), None, g.B, g.S, g.F,
                                           g.hop, g.n_mel, _CLIP, s), "melloss_terms")
            if want_t:
                xmel = torch.empty(g.B, g.n_mel, g.F, **f32)
        else:
            lens_k = lens
            spec, melp = _forward_chain(g, [x], lens, lens, fb, mb)
            tmel, Ft = target, int(target.shape[2])
        part = torch.empty(g.rows, **f32)
        check(lib.radmmm_melloss_terms(ptr(melp), g.ldn, ptr(lens), ptr(frames), ptr(tmel), Ft, ptr(xmel), ptr(part), g.B, g.S, g.F,
                                       g.hop, g.n_mel, _CLIP, s), "melloss_terms")
        out = torch.empty(1, **f32)
        norm = torch.empty(1, device=dev, dtype=torch.float64)
        check(lib.radmmm_melloss_finish(ptr(part), ptr(lens), ptr(frames), ptr(out), ptr(norm), g.B, g.S, g.F, Ft, g.hop, g.n_mel,
                                        s), "melloss_finish")
        ctx.g, ctx.Ft, ctx.bases, ctx.audio = g, Ft, (fb, mb), bool(target_is_audio)
        ctx.opt = (lens is not None, frames is not None, lens_k is not None and target_is_audio, xmel is not None)
        ctx.save_for_backward(spec, melp, tmel, norm, *[t for t in (lens, frames, lens_k if target_is_audio else None, xmel)
                                                         if t is not None])
        return out.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        spec, melp, tmel, norm, *rest = ctx.saved_tensors
        lens, frames, lens_k, xmel = (rest.pop(0) if has else None for has in ctx.opt)
        g, s = ctx.g, stream()
        want_x, want_t = ctx.needs_input_grad[0], bool(ctx.audio and ctx.needs_input_grad[1])
        if not (want_x or want_t):
            return (None,) * 6
        grad = f32c(grad)
        n_sig = int(want_x) + int(want_t)
        dmelp = torch.empty(n_sig * g.rows, g.ldn, device=grad.device, dtype=torch.float32)
        at = 0
        if want_x:
            check(lib.radmmm_melloss_bwd(ptr(melp), g.ldn, ptr(lens), ptr(frames), ptr(tmel), ctx.Ft, ptr(norm), ptr(grad), None,
                                         ptr(dmelp), g.B, g.S, g.F, g.hop, g.n_mel, _CLIP, s), "melloss_bwd")
            at = g.rows
        if want_t:                                              # d|a - b| / db = sign(b - a): the same kernel, roles swapped
            check(lib.radmmm_melloss_bwd(ptr(melp[g.rows:]), g.ldn, ptr(lens), ptr(frames), ptr(xmel), g.F, ptr(norm), ptr(grad),
                                         None, ptr(dmelp[at:]), g.B, g.S, g.F, g.hop, g.n_mel, _CLIP, s), "melloss_bwd")
        if n_sig == 2:
            sp, lk = spec, lens_k
        else:
            sp, lk = (spec[:g.rows] if want_x else spec[g.rows:]), lens
        dA = _backward_chain(g, dmelp, sp, lk, *ctx.bases)
        gx = _unframe(g, dA, lens) if want_x else None
        gt = _unframe(g, dA[at:] if want_x else dA, lens) if want_t else None
        return gx, gt, None, None, None, None


def _counts_on_device(v, B: int, dev: torch.device, what: str, lo: Optional[int] = None, hi: Optional[int] = None):
    """lens / frames -> an int32 device tensor [B] (host values are checked against (lo, hi] when given and go through
    pinned memory: no synchronisation); device tensors are taken as they are"""
    if v is None:
        return None
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"mel_loss: {what} on the device must be int32 or int64 (got {v.dtype})")
        out = v.reshape(-1).to(torch.int32)
    else:
        host = torch.as_tensor(v).reshape(-1).to(torch.int64)
        if lo is not None and host.numel() and (int(host.min()) <= lo or int(host.max()) > hi):
            raise ValueError(f"mel_loss: every item needs more than filter_length // 2 = {lo} and at most {hi} samples "
                             f"(got {host.tolist()})")
        out = host.to(torch.int32).pin_memory().to(dev, non_blocking=True)
    if out.numel() != B:
        raise ValueError(f"mel_loss: {what} has {out.numel()} entries for {B} items")
    return out.contiguous()


def _signal(t, what: str):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RadmmmError(f"mel_loss needs GPU tensors (there is no CPU path): {what}")
    if t.dim() == 3 and t.shape[1] == 1:
        t = t.reshape(t.shape[0], t.shape[2])
    if t.dim() != 2:
        raise ValueError(f"mel_loss: {what} {tuple(t.shape)} must be [B, S] or [B, 1, S]")
    return t


@fp32_region
def mel_spectrogram(y: torch.Tensor, stft: TacotronSTFT, lens=None) -> torch.Tensor:
    """y [B, S] or [B, 1, S] on the GPU -> log-mel [B, n_mel, 1 + S // hop] with a grad_fn (one autograd node): the
    differentiable form of stft.mel_spectrogram(y) (lens=None) and of stft.mel_spectrogram_ragged(y, lens) (lens: samples
    per item as an int32 / int64 device tensor, a host sequence, or None = S; frames past 1 + lens[b] // hop are exact
    zeros).  No range assert and no synchronisation.  Host lens must lie in (filter_length // 2, S]; device lens are the
    caller's promise, and the kernels stay inside every item whatever they hold."""
    y = _signal(y, "y")
    g = _Geometry(stft, *y.shape)
    lens = _counts_on_device(lens, g.B, y.device, "lens", g.h, g.S)
    return _MelFn.apply(y, lens, stft)


@fp32_region
def _mel_loss(stft: TacotronSTFT, x, target, lens, frames):
    x = _signal(x, "x")
    if not (isinstance(target, torch.Tensor) and target.is_cuda):
        raise RadmmmError("mel_loss needs GPU tensors (there is no CPU path): target")
    B, S = x.shape
    n_mel = int(stft.n_mel_channels)
    is_mel = target.dim() == 3 and not (target.shape[1] == 1 and n_mel != 1)
    if is_mel:
        if target.shape[0] != B or target.shape[1] != n_mel or target.shape[2] < 1:
            raise ValueError(f"mel_loss: a target mel must be [{B}, {n_mel}, Ft] (got {tuple(target.shape)})")
        if target.requires_grad and torch.is_grad_enabled():
            raise ValueError("mel_loss: a target mel receives no gradient here: detach it (an audio target may ask for one)")
    else:
        target = _signal(target, "target")
        if target.shape != x.shape:
            raise ValueError(f"mel_loss: x {tuple(x.shape)} and an audio target {tuple(target.shape)} must agree")
    g = _Geometry(stft, B, S, signals=1 if is_mel else 2)
    lens = _counts_on_device(lens, B, x.device, "lens", g.h, g.S)
    frames = _counts_on_device(frames, B, x.device, "frames")
    return _MelLossFn.apply(x, target, lens, frames, stft, not is_mel)


class MelSpectrogramLoss(nn.Module):
    """L1 between the log-mel of x and a target, over the valid frames (F.l1_loss there).

    MelSpectrogramLoss(stft=None, **tacotron_stft_kwargs): holds a TacotronSTFT.  The default is
    TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0): the `data_config` block of the reference's shipped configs
    (filter_length 1024, hop_length 256, win_length 1024, n_mel_channels 80, sampling_rate 22050, mel_fmin 0.0,
    mel_fmax 8000.0), which data.py's AudioDataset hands to TacotronSTFT and which made the generator's input mels.

    forward(x, target, lens=None, frames=None) -> 0-d fp32 device tensor.  x: audio [B, S] or [B, 1, S].  target: a mel
    [B, n_mel, Ft] in the reference layout (no gradient), or audio shaped like x (transformed by the same kernels with the
    same lens; it gets a gradient if it asks).  lens: samples per item (int32 / int64 device tensor, host sequence, None = S).
    frames: optional frame counts per item (a batch's out_lens), read clamped into [0, min(F, Ft)].  Item b enters with
    n[b] = min(1 + lens[b] // hop, Ft, frames[b]) frames; sum n = 0 gives loss 0 and gradient 0."""

    def __init__(self, stft: Optional[TacotronSTFT] = None, **tacotron_stft_kwargs):
        super().__init__()
        if stft is not None and tacotron_stft_kwargs:
            raise ValueError("MelSpectrogramLoss: give a TacotronSTFT or its arguments, not both")
        if stft is None:
            kw = dict(filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050, mel_fmin=0.0,
                      mel_fmax=8000.0)
            kw.update(tacotron_stft_kwargs)
            stft = TacotronSTFT(**kw)
        self.stft = stft

    def forward(self, x, target, lens=None, frames=None):
        return _mel_loss(self.stft, x, target, lens, frames)
