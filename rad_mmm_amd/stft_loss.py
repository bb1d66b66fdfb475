"""Multi-resolution STFT loss on the GPU, forward and backward (reference stft_loss.py: STFTLoss,
MultiResolutionSTFTLoss, used by loss.py RADTTSE2EGANLoss), with ragged batches and no device -> host read.

    loss_fn = MultiResolutionSTFTLoss()                       # fft 1024/2048/512, hop 120/240/50, win 600/1200/240
    sc, mag = loss_fn(x, y, lens=None)                        # x, y [B, T] or [B, C, T]; lens: len_ratios [B] or None

Per resolution (csrc/stft_loss.hip): radmmm_stftloss_frame cuts the reflect-padded frames of both signals
into one stacked frame matrix that holds only the `win` columns under the window, ONE radmmm_rowgemm_f32 launch (exact
fp32 MFMA) multiplies it with the windowed DFT basis of those columns, radmmm_stftloss_terms reduces every frame to three
partial sums and radmmm_stftloss_finish folds them into the two losses in fp64.  The backward is radmmm_stftloss_bwd
(gradient of the spectra), one row GEMM on the transposed basis and radmmm_stftloss_unframe (the adjoint of the framing in
gather form, no atomics).  Semantics are the reference's: torch.stft(center=True) reflect-pads at the padded length T,
F = 1 + T // hop frames, item b counts ceil(len_ratios[b] * F) of them, mag = sqrt(clamp(re^2 + im^2, 1e-7)).
One restriction: the reference is followed for len_ratios in [0, 1].  A count above F is read as F here, also in the
sum of the frame counts that normalises both losses, where the reference's lens.sum() would keep the excess.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import RadmmmError, check, f32c, fp32_region, lib, ptr, rowgemm, stream

_OPERAND_BYTES = 2 ** 31 - 2 ** 16     # the row GEMM's operands (and the kernels' matrices here) stay below 2 GiB


def stft_loss_basis(n_fft: int, win_length: int, window=None) -> np.ndarray:
    """[2 * (n_fft/2 + 1), roundup4(win)] fp32: audio_processing.windowed_dft_basis restricted to the `win` columns where
    the centre-padded window is not padding (left = (n_fft - win) // 2), zero in the pad columns.  Rows: re of bins
    0 .. n_fft/2, then im (the DFT's, -sin).  window: [win] values, default the reference's buffer
    torch.hann_window(win) (periodic, fp32).  Computed in float64 with the phase reduced in integers, rounded once."""
    cutoff = n_fft // 2 + 1
    left = (n_fft - win_length) // 2
    n = np.arange(win_length, dtype=np.int64) + left
    k = np.arange(cutoff, dtype=np.int64)
    ang = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft).astype(np.float64) / n_fft
    if window is None:
        window = torch.hann_window(win_length).numpy()
    w = np.asarray(window, dtype=np.float64).reshape(1, win_length)
    out = np.zeros((2 * cutoff, ops.round_up(win_length, 4)), dtype=np.float32)
    out[:cutoff, :win_length] = np.cos(ang) * w
    out[cutoff:, :win_length] = -np.sin(ang) * w
    return out


class _Resolution:
    """shape of one resolution for a signal of T samples"""

    def __init__(self, mod: "STFTLoss", rows_b: int, T: int):
        self.n_fft, self.hop, self.win, self.a_weighting = mod.fft_size, mod.shift_size, mod.win_length, int(mod.a_weighting)
        self.cutoff = self.n_fft // 2 + 1
        self.ldk = ops.round_up(self.win, 4)
        self.lds = ops.round_up(2 * self.cutoff, 4)
        self.F = 1 + T // self.hop
        self.rows = rows_b * self.F
        if T <= self.n_fft // 2:
            raise ValueError(f"STFTLoss: {T} samples cannot be reflect-padded by {self.n_fft // 2} (fft_size {self.n_fft} "
                             f"needs more than {self.n_fft // 2})")
        if 2 * self.rows * max(self.ldk, self.lds) * 4 >= _OPERAND_BYTES:
            raise ValueError(f"STFTLoss: {rows_b} x {T} samples at fft_size {self.n_fft}, hop {self.hop} exceed the row "
                             "GEMM's 2 GiB operand limit: split the batch")


class _STFTLossFn(torch.autograd.Function):
    """(x [R, T], y [R, T], frames int32 [resolutions, R] or None, modules) -> (sc, mag), the mean over the modules'
    resolutions, as one autograd node.  Saves, per resolution, the stacked spectra, the per-frame partials and the normalisers."""

    @staticmethod
    def forward(ctx, x, y, frames, mods):
        R, T = x.shape
        dev = x.device
        res = [_Resolution(m, R, T) for m in mods]              # every refusal comes before the first launch
        x, y = f32c(x.detach()), f32c(y.detach())
        s = stream()
        out = torch.empty(len(res), 2, device=dev, dtype=torch.float32)
        norm = torch.empty(len(res), 4, device=dev, dtype=torch.float64)
        saved = []
        for i, (m, r) in enumerate(zip(mods, res)):
            basis = m._basis_on(dev)
            fr = frames[i] if frames is not None else None
            A = torch.empty(2 * r.rows, r.ldk, device=dev, dtype=torch.float32)
            for sig, dst in ((x, A), (y, A[r.rows:])):
                check(lib.radmmm_stftloss_frame(ptr(sig), T, ptr(fr), ptr(dst), r.ldk, R, T, r.F, r.n_fft, r.hop, r.win,
                                                s), "stftloss_frame")
            spec = torch.empty(2 * r.rows, r.lds, device=dev, dtype=torch.float32)
            rowgemm(A=A, lda=r.ldk, B=basis, ldb=r.ldk, b_tap_stride=0, C=spec, ldc=r.lds, M=2 * r.rows, N=2 * r.cutoff,
                    K=r.win, T=r.F)
            part = torch.empty(r.rows, 4, device=dev, dtype=torch.float32)
            check(lib.radmmm_stftloss_terms(ptr(spec), ptr(spec[r.rows:]), r.lds, ptr(fr), ptr(part), R, r.F, r.cutoff,
                                            r.a_weighting, s), "stftloss_terms")
            check(lib.radmmm_stftloss_finish(ptr(part), ptr(fr), ptr(out[i]), ptr(norm[i]), R, r.F, r.cutoff, s),
                  "stftloss_finish")
            saved += [spec, part]
        ctx.mods, ctx.res, ctx.shape = mods, res, (R, T)
        ctx.has_frames = frames is not None
        ctx.save_for_backward(norm, *([frames] if frames is not None else []), *saved)
        if len(res) == 1:
            return out[0, 0].clone(), out[0, 1].clone()
        return out[:, 0].mean(), out[:, 1].mean()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sc, g_mag):
        norm, *rest = ctx.saved_tensors
        frames = rest.pop(0) if ctx.has_frames else None
        want = [ctx.needs_input_grad[0], ctx.needs_input_grad[1]]
        R, T = ctx.shape
        dev = norm.device
        s = stream()
        g_sc, g_mag = f32c(g_sc), f32c(g_mag)
        grads = [torch.empty(R, T, device=dev, dtype=torch.float32) if w else None for w in want]
        n_sig = sum(want)
        for i, (m, r) in enumerate(zip(ctx.mods, ctx.res)):
            spec, part = rest[2 * i], rest[2 * i + 1]
            fr = frames[i] if frames is not None else None
            dspec = torch.empty(n_sig * r.rows, r.lds, device=dev, dtype=torch.float32)
            d_of = [None, None]
            at = 0
            for j in range(2):
                if want[j]:
                    d_of[j] = at
                    at += r.rows
            check(lib.radmmm_stftloss_bwd(ptr(spec), ptr(spec[r.rows:]), r.lds, ptr(part), ptr(norm[i]), ptr(fr),
                                          ptr(g_sc), ptr(g_mag), 1.0 / len(ctx.res),
                                          ptr(dspec[d_of[0]:]) if want[0] else None, ptr(dspec[d_of[1]:]) if want[1] else None,
                                          R, r.F, r.cutoff, r.a_weighting, s), "stftloss_bwd")
            dA = torch.empty(n_sig * r.rows, r.ldk, device=dev, dtype=torch.float32)
            rowgemm(A=dspec, lda=r.lds, B=m._basis_on(dev), ldb=r.ldk, b_tap_stride=0, b_layout=1, C=dA, ldc=r.ldk,
                    M=n_sig * r.rows, N=r.win, K=2 * r.cutoff, T=r.F)
            for j in range(2):
                if want[j]:
                    check(lib.radmmm_stftloss_unframe(ptr(dA[d_of[j]:]), r.ldk, ptr(fr), ptr(grads[j]), T, R, T, r.F,
                                                      r.n_fft, r.hop, r.win, int(i > 0), s), "stftloss_unframe")
        return grads[0], grads[1], None, None


def _ratios_on_device(lens, rows_b: int, batch: int, dev: torch.device) -> Optional[torch.Tensor]:
    """len_ratios -> a device tensor [rows_b] in its own dtype (host values go through pinned memory, no synchronisation);
    [B] ratios for a [B, C, T] input repeat per channel"""
    if lens is None:
        return None
    if not (isinstance(lens, torch.Tensor) and lens.is_cuda):
        host = torch.as_tensor(lens)
        if not host.is_floating_point():
            host = host.float()
        lens = host.reshape(-1).pin_memory().to(dev, non_blocking=True)
    lens = lens.reshape(-1)
    if lens.numel() == batch and rows_b != batch:
        lens = lens.repeat_interleave(rows_b // batch)
    if lens.numel() != rows_b:
        raise ValueError(f"lens has {lens.numel()} entries for {rows_b} signals")
    return lens


@fp32_region
def _loss(mods: Sequence["STFTLoss"], x: torch.Tensor, y: torch.Tensor, lens):
    if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.is_cuda and y.is_cuda):
        raise RadmmmError("STFTLoss needs GPU tensors (there is no CPU path)")
    if x.shape != y.shape or x.dim() not in (2, 3):
        raise ValueError(f"STFTLoss: x {tuple(x.shape)} and y {tuple(y.shape)} must both be [B, T] or [B, C, T]")
    batch = x.shape[0]
    if x.dim() == 3:
        x, y = x.reshape(-1, x.shape[2]), y.reshape(-1, y.shape[2])
    R, T = x.shape
    for m in mods:                                              # every refusal comes before the first launch
        _Resolution(m, R, T)
    ratios = _ratios_on_device(lens, R, batch, x.device)
    frames = None
    if ratios is not None:                                      # [resolutions, R] int32: every hop has its own frame count
        frames = torch.stack([_frame_counts(ratios, 1 + T // m.shift_size) for m in mods])
    return _STFTLossFn.apply(x, y, frames, list(mods))


def _frame_counts(ratios: torch.Tensor, F: int) -> torch.Tensor:
    """the reference's (len_ratios * y_mag.shape[1]).ceil().long(), in len_ratios' dtype on the device, as int32 (the
    kernels read it clamped to [0, F])"""
    return (ratios * F).ceil().to(torch.int32)


class STFTLoss(nn.Module):
    """STFTLoss(fft_size, shift_size, win_length, window, sampling_rate, a_weighting) of stft_loss.py:218-258: one
    resolution.  forward(x, y, lens=None) -> (spectral convergence, log STFT magnitude), 0-d fp32 device tensors."""

    def __init__(self, fft_size=1024, shift_size=120, win_length=600, window="hann_window", sampling_rate=22050,
                 a_weighting=False):
        super().__init__()
        if window != "hann_window":
            raise ValueError(f"STFTLoss: window {window!r} is not supported (only 'hann_window')")
        self.fft_size, self.shift_size, self.win_length = int(fft_size), int(shift_size), int(win_length)
        if self.fft_size < 2 or self.fft_size % 2 or not 1 <= self.win_length <= self.fft_size or self.shift_size < 1:
            raise ValueError(f"STFTLoss: needs an even fft_size >= 2, 1 <= win_length <= fft_size and shift_size >= 1 (got "
                             f"{fft_size}, {win_length}, {shift_size})")
        self.sampling_rate = sampling_rate
        self.a_weighting = bool(a_weighting)
        self.register_buffer("window", torch.hann_window(self.win_length))
        self.register_buffer("basis", None, persistent=False)
        self.register_load_state_dict_post_hook(lambda module, _: setattr(module, "basis", None))

    def _basis_on(self, dev: torch.device) -> torch.Tensor:
        """the DFT basis times the `window` buffer on `dev`, built at the first use there and after a load_state_dict
        (the two copies wait for the device: the first call is not free of synchronisation, every later one is)"""
        if self.basis is None or self.basis.device != dev or self.basis.dtype != torch.float32:   # module.double() / .half()
            w = self.window.detach().double().cpu().numpy()
            self.basis = torch.from_numpy(stft_loss_basis(self.fft_size, self.win_length, w)).to(dev)
        return self.basis

    def forward(self, x, y, lens=None):
        return _loss([self], x, y, lens)


class MultiResolutionSTFTLoss(nn.Module):
    """MultiResolutionSTFTLoss of stft_loss.py:261-314: the mean of STFTLoss over the resolutions; state_dict keys
    stft_losses.N.window.  forward(x, y, lens=None): x, y [B, T] or [B, C, T] (viewed as [B*C, T]) on the GPU; lens the
    reference's len_ratios [B] (device tensor: no synchronisation; host values are copied through pinned memory) or None.
    Gradients are computed for whichever of x, y requires them."""

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240],
                 window="hann_window", sampling_rate=22050, a_weighting=False):
        super().__init__()
        if not len(fft_sizes) == len(hop_sizes) == len(win_lengths):
            raise ValueError("MultiResolutionSTFTLoss: fft_sizes, hop_sizes and win_lengths differ in length")
        self.stft_losses = nn.ModuleList(
            STFTLoss(fs, ss, wl, window, sampling_rate=sampling_rate, a_weighting=a_weighting)
            for fs, ss, wl in zip(fft_sizes, hop_sizes, win_lengths))

    def forward(self, x, y, lens=None):
        return _loss(list(self.stft_losses), x, y, lens)
