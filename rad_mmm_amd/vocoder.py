"""HiFi-GAN generator + STFT denoiser, batched on the GPU: mel -> waveform (reference vocoders/hifigan_models.py:104-247,
vocoders/hifigan_denoiser.py:25-58, audio_processing.py:195-291, vocoders/vocoder_utils.py:35-48, 104-132).

The reference vocodes one utterance at a time on the CPU.  Here a batch [B, 80, T] with per-item lengths goes through
one launch sequence; item b equals a call with item b alone (every layer treats rows at or past the item's length,
times the stage's upsample product, as zeros, and the denoiser reflects at the item's own length) and everything past
its length is exactly 0.

Layout: channels-last rows ([B*T, C] fp32, row r = b*T + t) as in the rest of the package.  Every convolution is a
radmmm_rowgemm_f32 launch (exact fp32 MFMA):
  * Conv1d(k, dilation d): taps = k, dil = d, length-masked operand rows.
  * ConvTranspose1d(k, u, p): in channels-last the u output rows i*u .. i*u+u-1 are contiguous, so the layer is ONE
    row GEMM with N = u*Cout over a window of input rows, reading input row i and writing the [rows][u*Cout] view of
    the output; its weight is packed once (pack_polyphase, zeros where a tap does not reach a phase).
  * the inverse STFT is the same polyphase GEMM (u = hop, k = n_fft, N = hop), the trim folded into the packing.
leaky_relu of a conv's operand, conv_post + tanh, the reflect pad, the bin rescale, the window-sum division and the
normalisation are kernels of csrc/vocoder.hip.

That is precision "fp32", the default.  With HiFiGANGenerator.precision "f16" (inference only, opt-in) every resblock conv
of a stage whose width the kernel takes is ONE radmmm_voc_conv_f16 launch (csrc/vocoder_f16.hip): fp16 operands, fp32
accumulation on the f16 matrix cores, the leaky-relu applied while the input tile is loaded, so no radmmm_voc_lrelu
launch is left inside a resblock.  conv_pre, the transposed convs, conv_post and the denoiser stay fp32, and so does a
stage the kernel does not take (widths such as 8 or 4): precision_plan() says what a config gets.
"""
from __future__ import annotations

import json
import warnings
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import RadmmmError, check, f32c, fp32_region, lib, ptr, rowgemm, stream, voc_conv_f16, voc_conv_f16_plan
from .audio_processing import _hann_periodic, windowed_dft_basis

LRELU_SLOPE = 0.1          # hifigan_models.py:52 (the final leaky_relu before conv_post uses torch's default 0.01)
POST_SLOPE = 0.01
N_MEL = 80
PRECISIONS = ("fp32", "f16")           # HiFiGANGenerator.precision: how inference runs the resblock convs
_OPERAND_BYTES = 2 ** 31 - 2 ** 16     # the row GEMM's 16-row fast path needs operands below 2 GiB


def get_padding(kernel_size: int, dilation: int = 1) -> int:
    return int((kernel_size * dilation - dilation) / 2)


def _cfg(h, key, default=None):
    if isinstance(h, dict):
        return h.get(key, default)
    return getattr(h, key, default)


def fold_weight_norm(v: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """torch weight_norm with its default dim = 0: w = g * v / ||v[i]|| over all dimensions but the first.  For a
    ConvTranspose1d weight [Cin, Cout, k] the first dimension is the INPUT channel.  Any device (the CPU restatement of
    what radmmm_weightnorm_fwd computes)."""
    n = v.reshape(v.shape[0], -1).norm(dim=1)
    shape = (-1,) + (1,) * (v.dim() - 1)
    return v * (g.reshape(shape) / n.reshape(shape))


def polyphase_shifts(k: int, u: int, p: int, off: int = 0) -> int:
    """half width h of the tap window (taps = 2h + 1) of pack_polyphase"""
    h = 0
    for j in range(k):
        r = (j - p) % u
        s = (r + p - j) // u
        h = max(h, abs(off + s))
    return h


def pack_polyphase(w: torch.Tensor, u: int, p: int, off: int = 0, ldk: Optional[int] = None) -> torch.Tensor:
    """ConvTranspose1d weight w [Cin, Cout, k] (stride u, padding p) -> Wp [taps, u*Cout, ldk] (K-contiguous, zero
    padded to ldk >= Cin) such that output sample o = (g + off) * u + r is

        y[o, co] = sum_tap sum_ci x[g + tap - taps//2, ci] * Wp[tap, r*Cout + co, ci]

    i.e. a centred `taps`-tap row GEMM over the input rows writing output row group g.  Output o receives input i
    through tap j = o + p - i*u; with o = q*u + r and i = q + s that is j = r + p - s*u.  off shifts the output rows
    by whole groups (the inverse STFT's n_fft/2 trim).  Works on any device."""
    Cin, Cout, k = w.shape
    ldk = ldk or Cin
    h = polyphase_shifts(k, u, p, off)
    j = torch.arange(k, device=w.device)        # on w's device: no host -> device copy, so a training step can call it
    r = (j - p) % u
    s = (r + p - j) // u
    tap = off + s + h
    Wp = torch.zeros(2 * h + 1, u, Cout, ldk, dtype=w.dtype, device=w.device)
    Wp[tap, r, :, :Cin] = w.permute(2, 1, 0)
    return Wp.reshape(2 * h + 1, u * Cout, ldk)


def remap_old_keys(state_dict: dict) -> dict:
    """Generator.load_state_dict's remap of old checkpoints (hifigan_models.py:207-219): a 5-part key
    resblocks.N.<convs>.<n>.<param> becomes resblocks.{N//3}.{N%3}.<convs>.<n>.<param>."""
    out = {}
    for k, v in state_dict.items():
        nk = k
        if "resblocks" in k:
            parts = k.split(".")
            if len(parts) == 5:
                layer = int(parts[1])
                nk = f"resblocks.{layer // 3}.{layer % 3}.{'.'.join(parts[2:])}"
        out[nk] = v
    return out


def _wn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.weight_norm(m)


def _unwn(m: nn.Module) -> None:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nn.utils.remove_weight_norm(m)


class _ResBlock1(nn.Module):
    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        self.kernel_size, self.dilation = kernel_size, tuple(dilation)
        self.convs1 = nn.ModuleList([_wn(nn.Conv1d(channels, channels, kernel_size, 1, dilation=d,
                                                   padding=get_padding(kernel_size, d))) for d in dilation])
        self.convs2 = nn.ModuleList([_wn(nn.Conv1d(channels, channels, kernel_size, 1, dilation=1,
                                                   padding=get_padding(kernel_size, 1))) for _ in dilation])

    def plan(self):
        """[(conv, dilation, lrelu its output, residual add)] in order"""
        out = []
        for c1, c2, d in zip(self.convs1, self.convs2, self.dilation):
            out.append((c1, d, True, False))
            out.append((c2, 1, False, True))
        return out


class _ResBlock2(nn.Module):
    def __init__(self, channels, kernel_size=3, dilation=(1, 3)):
        super().__init__()
        self.kernel_size, self.dilation = kernel_size, tuple(dilation)
        self.convs = nn.ModuleList([_wn(nn.Conv1d(channels, channels, kernel_size, 1, dilation=d,
                                                  padding=get_padding(kernel_size, d))) for d in dilation])

    def plan(self):
        return [(c, d, False, True) for c, d in zip(self.convs, self.dilation)]


def _conv_weight(m: nn.Module) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    if hasattr(m, "weight_g"):
        return m.weight_v, m.weight_g
    return m.weight, None


def _lens_arg(lens, B: int, T: int, dev: torch.device):
    """-> (device int32 [B], host int64 [B] or None).  Host lengths are copied through pinned memory without a
    synchronisation; device lengths are used as they are."""
    if lens is None:
        host = torch.full((B,), T, dtype=torch.int64)
    elif isinstance(lens, torch.Tensor) and lens.is_cuda:
        return lens.to(torch.int32), None
    else:
        host = torch.as_tensor(lens, dtype=torch.int64).reshape(-1).cpu()
    if host.numel() != B:
        raise ValueError(f"lens has {host.numel()} entries for a batch of {B}")
    if bool((host < 1).any()) or bool((host > T).any()):
        raise ValueError(f"lens must lie in [1, {T}], got {host.tolist()}")
    return _to_device(host, dev), host


def _to_device(host: torch.Tensor, dev: torch.device) -> torch.Tensor:
    return host.to(torch.int32).pin_memory().to(dev, non_blocking=True)


class HiFiGANGenerator(nn.Module):
    """HiFi-GAN Generator(h) (hifigan_models.py:172-247): same sub-module and state_dict names (conv_pre, ups.{i},
    resblocks.{i}.{j}.convs1/convs2/convs.{n}, conv_post with .weight_g/.weight_v/.bias), forward on the GPU.

    forward(mel [B, 80, T], lens=None, precision=None) -> audio [B, 1, T * prod(upsample_rates)], zero past lens[b] * hop.
    lens: host (list / CPU tensor: no synchronisation) or device lengths in mel frames.
    precision ("fp32", the default, or "f16"; the attribute `precision`, or per call): how inference runs the resblock
    convs.  "f16": fp16 operands and fp32 accumulation on the f16 matrix cores in every stage the kernel takes
    (precision_plan()); the rest of the model, and a training step, stay fp32."""

    def __init__(self, h):
        super().__init__()
        blur = _cfg(h, "gaussian_blur", None) or {"p_blurring": 0.0}
        if float(blur.get("p_blurring", 0.0)) > 0.0:
            raise ValueError("HiFiGANGenerator: the Gaussian blur augmentation (p_blurring > 0) is not supported")
        self.upsample_rates = [int(u) for u in _cfg(h, "upsample_rates")]
        self.upsample_kernel_sizes = [int(k) for k in _cfg(h, "upsample_kernel_sizes")]
        self.resblock_kernel_sizes = [int(k) for k in _cfg(h, "resblock_kernel_sizes")]
        self.resblock_dilation_sizes = [list(d) for d in _cfg(h, "resblock_dilation_sizes")]
        c0 = int(_cfg(h, "upsample_initial_channel"))
        self.resblock_type = str(_cfg(h, "resblock"))
        if self.resblock_type not in ("1", "2"):
            raise ValueError(f"resblock must be '1' or '2', got {self.resblock_type!r}")
        self.num_kernels = len(self.resblock_kernel_sizes)
        self.num_upsamples = len(self.upsample_rates)
        for u, k in zip(self.upsample_rates, self.upsample_kernel_sizes):
            if (k - u) % 2:
                raise ValueError(f"upsample kernel {k} with rate {u}: output length is not T*u (k - u must be even)")
        for k in self.resblock_kernel_sizes:
            if k % 2 == 0:
                raise ValueError(f"resblock kernel {k}: only odd kernels keep the length")
        for i in range(self.num_upsamples + 1):
            if (c0 >> i) % 4 or (c0 >> i) << i != c0:
                raise ValueError(f"upsample_initial_channel {c0}: every stage's width must be a multiple of 4")
        self.hop = int(np.prod(self.upsample_rates))
        self.conv_pre = _wn(nn.Conv1d(N_MEL, c0, 7, 1, padding=3))
        res = _ResBlock1 if self.resblock_type == "1" else _ResBlock2
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            self.ups.append(_wn(nn.ConvTranspose1d(c0 // (2 ** i), c0 // (2 ** (i + 1)), k, u, padding=(k - u) // 2)))
        self.resblocks = nn.ModuleList()
        ch = c0
        for i in range(self.num_upsamples):
            ch = c0 // (2 ** (i + 1))
            self.resblocks.append(nn.ModuleList([res(ch, k, d) for k, d in
                                                 zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)]))
        self.conv_post = _wn(nn.Conv1d(ch, 1, 7, 1, padding=3))
        self._folded = None
        self._folded_key = None
        self.precision = "fp32"

    def load_state_dict(self, state_dict, strict: bool = True):
        self._folded = None
        return super().load_state_dict(remap_old_keys(state_dict), strict=strict)

    def remove_weight_norm(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)) and hasattr(m, "weight_g"):
                _unwn(m)
        self._folded = None

    # ---- weights in the kernels' layout, folded once (again only when a parameter changed) --------------------
    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    @staticmethod
    def _fold_conv(m: nn.Module, ldw: int) -> torch.Tensor:
        """Conv1d -> W [taps, Cout, ldw] (radmmm_rowgemm_f32 layout 0)"""
        v, g = _conv_weight(m)
        if g is not None:
            return ops.weightnorm_fwd(f32c(v.detach()), f32c(g.detach()), ldw)[0]
        Cout, Cin, taps = v.shape
        W = torch.zeros(taps, Cout, ldw, device=v.device, dtype=torch.float32)
        W[:, :, :Cin] = v.detach().float().permute(2, 0, 1)
        return W

    def _fold(self):
        key = self._key()
        if self._folded is not None and self._folded_key == key:
            return self._folded
        f = {"pre": (self._fold_conv(self.conv_pre, N_MEL), f32c(self.conv_pre.bias.detach()))}
        ups = []
        for m, u, k in zip(self.ups, self.upsample_rates, self.upsample_kernel_sizes):
            v, g = _conv_weight(m)
            Cin, Cout, _ = v.shape
            if g is not None:       # weight_norm dim 0 of a [Cin, Cout, k] weight: one norm per INPUT channel
                W = ops.weightnorm_fwd(f32c(v.detach()), f32c(g.detach()), Cout)[0]      # [k, Cin, Cout]
                w = W.permute(1, 2, 0)
            else:
                w = v.detach().float()
            Wp = pack_polyphase(w, u, (k - u) // 2).contiguous()
            ups.append((Wp, f32c(m.bias.detach()).repeat(u)))
        f["ups"] = ups
        f["res"] = [[[(self._fold_conv(c, c.in_channels), f32c(c.bias.detach()), c.kernel_size[0], d, act, add)
                      for c, d, act, add in blk.plan()] for blk in group] for group in self.resblocks]
        C = self.conv_post.in_channels
        ldw = ops.round_up(C, 4)
        f["post"] = (self._fold_conv(self.conv_post, ldw).reshape(-1).contiguous(), f32c(self.conv_post.bias.detach()))
        self._folded, self._folded_key = f, key
        return f

    # ---- precision "f16": which stages run on radmmm_voc_conv_f16, and their fp16 weights -----------------------------
    @staticmethod
    def _check_precision(precision: str) -> str:
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r}: one of {PRECISIONS}")
        return precision

    def _mode(self, precision: Optional[str] = None) -> str:
        """the mode a call runs in (None: the attribute), a known name; `precision` means inference only: in training
        mode with grad enabled the step is the fp32 step whatever the name says"""
        mode = self._check_precision(self.precision if precision is None else precision)
        return "fp32" if self._train_active() else mode

    def precision_plan(self, precision: Optional[str] = None) -> list:
        """per stage (mode, reason): ("f16", "") when every resblock conv of the stage reaches a radmmm_voc_conv_f16
        kernel, else ("fp32", why).  Host only (the kernel family's own plan query decides), any device."""
        mode = self._check_precision(self.precision if precision is None else precision)
        out = []
        a = 0x10000                                      # stands for an address: the plan query dereferences nothing
        for group in self.resblocks:
            if mode == "fp32":
                out.append(("fp32", "precision 'fp32'"))
                continue
            why = ""
            for blk in group:
                for c, d, _, _ in blk.plan():
                    C = c.in_channels
                    ld = ops.round_up(C, 8)
                    if not voc_conv_f16_plan(X=a, ldx=ld, Wh=a, ldw=ld, Y=2 * a, ldy=ld, B=1, T=1, C=C, taps=c.kernel_size[0],
                                             dil=d, bias=a):
                        why = why or lib.radmmm_last_error().decode()
            out.append(("fp32", why) if why else ("f16", ""))
        return out

    def _f16_weights(self, f: dict, i: int) -> list:
        """fp16(W * ops.W_SCALE) of stage i's folded resblock weights, [taps, C, C] each, per block in conv order.  Made
        once per fold and kept inside it, so they go when a parameter changes."""
        cache = f.setdefault("f16", {})
        if i not in cache:
            cache[i] = [[ops.split_f16(Wc.view(-1, Wc.shape[2]), Wc.shape[2], ops.W_SCALE, Wc.shape[2], nprod=1)[0]
                         for Wc, _, _, _, _, _ in blk] for blk in f["res"][i]]
        return cache[i]

    # ---- training: the same forward under one autograd node whose backward is the HIP path -------------------------
    def _train_active(self) -> bool:
        return self.training and torch.is_grad_enabled()

    def _conv_names(self):
        """every conv's module path, in the order of the forward pass (= of the autograd node's weight arguments)"""
        path = {id(m): n for n, m in self.named_modules()}
        names = ["conv_pre"]
        for up, group in zip(self.ups, self.resblocks):
            names.append(path[id(up)])
            for blk in group:
                names += [path[id(c)] for c, _, _, _ in blk.plan()]
        return names + ["conv_post"]

    def _train_weights(self):
        """(weight, bias) of every conv in _conv_names() order, reference layouts; a weight-normed conv's weight is folded
        with torch ops, so autograd carries the node's gradient of the folded weight on to weight_g and weight_v"""
        out = []
        for n in self._conv_names():
            m = self.get_submodule(n)
            out.append(fold_weight_norm(m.weight_v.float(), m.weight_g.float()) if "weight_g" in m._parameters
                       else m.weight)
            out.append(m.bias)
        return out

    def _check_train_shape(self, B: int, T: int) -> None:
        """the backward's GEMM operands ([rows, C] gradients, the [rows, u * Cout] view of a transposed conv's output
        gradient) must stay below the row GEMM's 2 GiB operand limit: checked before any launch"""
        rows, C = B * T, self.conv_pre.out_channels
        worst = rows * max(C, N_MEL)
        for u in self.upsample_rates:
            rows, C = rows * u, C // 2
            worst = max(worst, rows * C)
        if 4 * worst > _OPERAND_BYTES:
            raise ValueError(f"HiFiGANGenerator: a training step on {B} x {T} frames needs a GEMM operand of "
                             f"{4 * worst} bytes, above the row GEMM's limit of {_OPERAND_BYTES} (there is no chunking: "
                             "train on shorter segments or a smaller batch)")
        if self.conv_post.in_channels > 1024:
            raise ValueError("HiFiGANGenerator: conv_post's backward kernel holds at most 1024 channels")

    @fp32_region
    def forward(self, mel: torch.Tensor, lens=None, precision: Optional[str] = None) -> torch.Tensor:
        """In training mode with grad enabled, and when mel or a parameter requires grad, the audio carries a grad_fn
        whose backward runs in HIP (same audio bits as eval mode); otherwise the plain launch sequence.
        precision ("fp32" or "f16"; None: the attribute `precision`): how inference runs the resblock convs; a training
        step ignores it."""
        mode = self._mode(precision)
        if not mel.is_cuda:
            raise RadmmmError("HiFiGANGenerator needs a GPU tensor (there is no CPU path)")
        if mel.dim() != 3 or mel.shape[1] != N_MEL:
            raise ValueError(f"mel must be [B, {N_MEL}, T], got {tuple(mel.shape)}")
        dev = mel.device
        B, _, T = mel.shape
        lens_d, _ = _lens_arg(lens, B, T, dev)
        if self._train_active() and (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            self._check_train_shape(B, T)
            return _GeneratorFn.apply(self, f32c(mel), lens_d, *self._train_weights())
        return self._run(f32c(mel), lens_d, precision=mode)

    def _run(self, mel: torch.Tensor, lens_d: torch.Tensor, events: Optional[list] = None,
             tape: Optional[dict] = None, precision: str = "fp32") -> torch.Tensor:
        """events: a list that receives a recorded device event after conv_pre, each stage and conv_post (timing).
        tape (a training step, _GeneratorFn): the same launches with the same arguments, but every conv's A operand goes
        to a buffer of its own and is recorded in tape with the shapes the backward walk needs; the audio's bits do not
        depend on it.
        precision "f16" (never with a tape): the stages precision_plan marks "f16" run their resblock convs on
        radmmm_voc_conv_f16; everything else is the fp32 launch sequence unchanged."""
        B, _, T = mel.shape
        stage_mode = [m for m, _ in self.precision_plan(precision)] if tape is None else ["fp32"] * self.num_upsamples
        mark = (lambda: events.append(torch.cuda.Event(enable_timing=True)) or events[-1].record()) if events is not None \
            else (lambda: None)
        mark()
        f = self._fold()
        R, Tc, lc = B * T, T, lens_d
        xm = torch.empty(R, N_MEL, device=mel.device, dtype=torch.float32)
        check(lib.radmmm_squeeze_rows(ptr(mel), ptr(xm), B, N_MEL, T, 1, N_MEL, 0, stream()), "squeeze_rows")
        W, b = f["pre"]
        C = W.shape[1]
        x = torch.empty(R, C, device=mel.device, dtype=torch.float32)
        rowgemm(A=xm, lda=N_MEL, B=W, ldb=W.shape[2], b_tap_stride=W.stride(0), C=x, ldc=C, M=R, N=C, K=N_MEL,
                taps=W.shape[0], dil=1, T=Tc, lens=lc, a_mask_mode=1, bias=b, postmask=1)
        mark()
        div = 1.0
        for i, u in enumerate(self.upsample_rates):
            Wp, bp = f["ups"][i]
            Cin, Cout = C, C // 2
            a = torch.empty(R, Cin, device=mel.device, dtype=torch.float32)
            check(lib.radmmm_voc_lrelu(ptr(x), Cin, ptr(a), Cin, R, Cin, Tc, ptr(lc), div, LRELU_SLOPE, stream()),
                  "voc_lrelu")
            if tape is not None:
                tape["stages"].append({"a": a, "div": div, "R": R, "T": Tc, "lens": lc, "Cin": Cin, "Cout": Cout, "u": u,
                                       "blocks": []})
            xu = torch.empty(R * u, Cout, device=mel.device, dtype=torch.float32)
            rowgemm(A=a, lda=Cin, B=Wp, ldb=Wp.shape[2], b_tap_stride=Wp.stride(0), C=xu, ldc=u * Cout, M=R,
                    N=u * Cout, K=Cin, taps=Wp.shape[0], dil=1, T=Tc, lens=lc, a_mask_mode=1, bias=bp, postmask=1)
            R, Tc, C = R * u, Tc * u, Cout
            lc = lc * u
            xs = torch.empty(R, C, device=mel.device, dtype=torch.float32)
            a = torch.empty(R, C, device=mel.device, dtype=torch.float32)
            t = torch.empty(R, C, device=mel.device, dtype=torch.float32)
            bufs = [torch.empty(R, C, device=mel.device, dtype=torch.float32) for _ in range(2)]
            wh16 = self._f16_weights(f, i) if stage_mode[i] == "f16" else None
            for j, blk in enumerate(f["res"][i]):
                xc, nxt = xu, 0
                if wh16 is not None:           # c1 writes raw t; every conv applies the leaky-relu to what it loads
                    for n, (Wc, bc, k, d, act, add) in enumerate(blk):
                        last = n == len(blk) - 1
                        out = bufs[nxt] if add else t
                        voc_conv_f16(X=t if add and n > 0 and blk[n - 1][4] else xc, ldx=C, Wh=wh16[j][n], ldw=C, Y=out,
                                     ldy=C, B=B, T=Tc, C=C, taps=k, dil=d, lens=lc, bias=bc, add=xc if add else None,
                                     ldadd=C, Y2=xs if add and last else None, ldy2=C,
                                     y2_accum=1 if (add and last and j > 0) else 0, in_scale=1.0, in_slope=LRELU_SLOPE,
                                     acc_scale=1.0 / ops.W_SCALE)
                        if add:
                            xc, nxt = out, 1 - nxt
                    continue
                ops_j = []                     # tape: the A operand of every conv of this block, in order
                for n, (Wc, bc, k, d, act, add) in enumerate(blk):
                    if tape is not None:       # a buffer per operand instead of the shared pair
                        a = torch.empty(R, C, device=mel.device, dtype=torch.float32)
                        if not add:
                            t = torch.empty(R, C, device=mel.device, dtype=torch.float32)
                    if add:                    # x = conv(lrelu(...)) + x  (ResBlock1's c2, ResBlock2's convs)
                        src = t if n > 0 and blk[n - 1][4] else None
                        if src is None:
                            check(lib.radmmm_voc_lrelu(ptr(xc), C, ptr(a), C, R, C, Tc, ptr(lc), 1.0, LRELU_SLOPE,
                                                       stream()), "voc_lrelu")
                            src = a
                        out = bufs[nxt]
                        last = n == len(blk) - 1
                        rowgemm(A=src, lda=C, B=Wc, ldb=Wc.shape[2], b_tap_stride=Wc.stride(0), C=out, ldc=C, M=R,
                                N=C, K=C, taps=k, dil=d, T=Tc, lens=lc, a_mask_mode=1, bias=bc, postmask=1,
                                add=xc, ldadd=C, C2=xs if last else None, ldc2=C, c2_accum=1 if (last and j > 0) else 0)
                        xc, nxt = out, 1 - nxt
                        ops_j.append(src)
                    else:                      # ResBlock1's c1: t = lrelu(c1(lrelu(x)))
                        check(lib.radmmm_voc_lrelu(ptr(xc), C, ptr(a), C, R, C, Tc, ptr(lc), 1.0, LRELU_SLOPE,
                                                   stream()), "voc_lrelu")
                        rowgemm(A=a, lda=C, B=Wc, ldb=Wc.shape[2], b_tap_stride=Wc.stride(0), C=t, ldc=C, M=R, N=C,
                                K=C, taps=k, dil=d, T=Tc, lens=lc, a_mask_mode=1, bias=bc, postmask=1)
                        check(lib.radmmm_voc_lrelu(ptr(t), C, ptr(t), C, R, C, Tc, ptr(lc), 1.0, LRELU_SLOPE,
                                                   stream()), "voc_lrelu")
                        ops_j.append(a)
                if tape is not None:
                    tape["stages"][-1]["blocks"].append(ops_j)
            x = xs
            div = float(self.num_kernels)
            mark()
        Wpost, bpost = f["post"]
        audio = torch.empty(B, Tc, device=mel.device, dtype=torch.float32)
        check(lib.radmmm_voc_conv_post(ptr(x), C, ptr(Wpost), Wpost.numel() // 7, ptr(bpost), ptr(audio), R, C, 7, Tc,
                                       ptr(lc), div, POST_SLOPE, stream()), "voc_conv_post")
        mark()
        if tape is not None:
            tape.update(f=f, xm=xm, x=x, div=div, R=R, T=Tc, lens=lc, C=C)
        return audio.view(B, 1, Tc)


def _unpack_polyphase(P: torch.Tensor, Cout: int, k: int, u: int, p: int) -> torch.Tensor:
    """the inverse of pack_polyphase (offset 0) for a gradient: P [taps, u*Cout, Cin] -> [Cin, Cout, k]"""
    taps = P.shape[0]
    j = torch.arange(k, device=P.device)
    r = (j - p) % u
    tap = (r + p - j) // u + taps // 2
    return P.view(taps, u, Cout, P.shape[2])[tap, r].permute(2, 1, 0)


def convtranspose_grads(gy: torch.Tensor, a: torch.Tensor, Wp: torch.Tensor, k: int, u: int, R: int, T: int, lens):
    """Backward of the polyphase row GEMM of ConvTranspose1d(Cin, Cout, k, u, (k - u) // 2).  gy [R * u, Cout]: the
    gradient of its output rows (zeros at and past lens[b] * u); a [R, Cin]: the rows it read; Wp: its packed weight
    [taps, u * Cout, Cin].  -> (weight gradient [Cin, Cout, k], bias gradient [Cout], gradient of a [R, Cin]).  The
    weight gradient is radmmm_wgrad_f32 over the [R, u * Cout] view of gy, un-packed; the bias gradient the column sum
    of that view folded over u; the data gradient ONE row GEMM on the transposed packed weight with flipped taps."""
    from .waveglow import _colsum, _wgrad          # (waveglow imports this module)
    taps, N, Cin = Wp.shape
    Cout = N // u
    P = _wgrad(gy, N, N, a, Cin, Cin, R, T, lens, taps, 1, 1)
    gw = _unpack_polyphase(P, Cout, k, u, (k - u) // 2)
    gb = _colsum(gy, N, R, N).view(u, Cout).sum(0)
    ga = torch.empty(R, Cin, device=gy.device, dtype=torch.float32)
    rowgemm(A=gy, lda=N, B=Wp, ldb=Wp.shape[2], b_tap_stride=Wp.stride(0), b_layout=1, C=ga, ldc=Cin, M=R, N=Cin, K=N,
            taps=taps, dil=1, sign=-1, T=T, lens=lens, a_mask_mode=1, postmask=1)
    return gw, gb, ga


class _GeneratorFn(torch.autograd.Function):
    """HiFiGANGenerator.forward as one autograd node.  Inputs: the module, mel [B, 80, T], lens (device int32, frames),
    then (weight, bias) of every conv in _conv_names() order, reference layouts, weight norm already folded.  The forward
    is _run with a tape: it keeps every conv's A operand (the masked leaky-relu rows the conv read, 4 bytes per row and
    channel), the last stage's sum and the audio.  The backward walks the convs in reverse, channels-last rows
    throughout: per conv a data-gradient row GEMM on the transposed weight with flipped taps, a split-K
    weight gradient, a column sum for the bias and radmmm_voc_lrelu_bwd for the derivative factor (a > 0 is its
    switch) and the residual add."""

    @staticmethod
    def forward(ctx, model, mel, lens_d, *weights):
        tape = {"stages": []}
        audio = model._run(f32c(mel.detach()), lens_d, tape=tape)
        ctx.model, ctx.tape, ctx.mel_shape = model, tape, tuple(mel.shape)
        ctx.save_for_backward(audio)
        return audio

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_audio):
        from .waveglow import _colsum, _wgrad          # (waveglow imports this module)
        model, tape = ctx.model, ctx.tape
        audio, = ctx.saved_tensors
        f = tape["f"]
        dev = audio.device
        s = stream()
        grads = {}

        def empty(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)

        def conv_grads(name, gy, A, W, k, d, R, T, lens, want_data=True):
            """gy [R, Cout], the gradient of a conv's output, and its operand A [R, Cin] -> weight and bias gradients
            into grads; returns the gradient of A (before the derivative factor of the leaky relu that produced A)"""
            Cout, Cin = W.shape[1], A.shape[1]
            grads[name] = (_wgrad(gy, Cout, Cout, A, Cin, Cin, R, T, lens, k, d, 1).permute(1, 2, 0),
                           _colsum(gy, Cout, R, Cout))
            if not want_data:
                return None
            dA = empty(R, Cin)
            rowgemm(A=gy, lda=Cout, B=W, ldb=W.shape[2], b_tap_stride=W.stride(0), b_layout=1, C=dA, ldc=Cin, M=R,
                    N=Cin, K=Cout, taps=k, dil=d, sign=-1, T=T, lens=lens, a_mask_mode=1, postmask=1)
            return dA

        def lrelu_bwd(gy, A, gx, R, C, T, lens, div, accum):
            check(lib.radmmm_voc_lrelu_bwd(ptr(gy), C, ptr(A), C, ptr(gx), C, R, C, T, ptr(lens), div, LRELU_SLOPE,
                                           int(accum), s), "voc_lrelu_bwd")

        names = model._conv_names()
        # conv_post + tanh: the gradient of the last stage's sum, of conv_post's weight and of its bias
        R, T, lens, C = tape["R"], tape["T"], tape["lens"], tape["C"]
        Wpost, _ = f["post"]
        ldw = Wpost.numel() // 7
        gx, dw, db = empty(R, C), empty(7 * ldw), empty(1)
        scratch = empty(int(lib.radmmm_voc_conv_post_bwd_scratch_floats(R, C, 7, ldw)))
        check(lib.radmmm_voc_conv_post_bwd(ptr(tape["x"]), C, ptr(Wpost), ldw, ptr(audio), ptr(f32c(g_audio)), ptr(gx),
                                           C, ptr(dw), ptr(db), ptr(scratch), R, C, 7, T, ptr(lens), tape["div"],
                                           POST_SLOPE, s), "voc_conv_post_bwd")
        grads["conv_post"] = (dw.view(7, ldw)[:, :C].t()[None], db)
        pos = len(names) - 1
        for i in reversed(range(model.num_upsamples)):
            st = tape["stages"][i]
            nblk = sum(len(b) for b in f["res"][i])
            pos -= nblk
            first = pos                                  # names[first]: the first conv of this stage's first block
            total = None
            off = nblk
            for j in reversed(range(len(f["res"][i]))):
                blk, A_ops = f["res"][i][j], st["blocks"][j]
                off -= len(blk)
                # the stage's sum fans out to every block; the last block walked (j = 0) consumes gx itself
                g = gx.clone() if j > 0 else gx
                gy = g
                for n in reversed(range(len(blk))):
                    Wc, _, k, d, act, add = blk[n]
                    dA = conv_grads(names[first + off + n], gy, A_ops[n], Wc, k, d, R, T, lens)
                    if add and n > 0 and blk[n - 1][4]:  # the operand is c1's activated output: its gradient feeds c1
                        lrelu_bwd(dA, A_ops[n], dA, R, C, T, lens, 1.0, False)
                        gy = dA
                    else:                                # the operand is lrelu(x): x's gradient gains dA * lrelu'
                        lrelu_bwd(dA, A_ops[n], g, R, C, T, lens, 1.0, True)
                        gy = g
                total = g if total is None else total.add_(g)
            # the transposed conv: one row GEMM over the packed polyphase weight on the [rows, u * Cout] view
            pos -= 1
            u, Cin, Ru, Tu, lu = st["u"], st["Cin"], st["R"], st["T"], st["lens"]
            gw, gb, gx = convtranspose_grads(total, st["a"], f["ups"][i][0], model.upsample_kernel_sizes[i], u, Ru, Tu, lu)
            grads[names[pos]] = (gw, gb)
            lrelu_bwd(gx, st["a"], gx, Ru, Cin, Tu, lu, st["div"], False)
            R, T, lens, C = Ru, Tu, lu, Cin
        Wpre, _ = f["pre"]
        dxm = conv_grads("conv_pre", gx, tape["xm"], Wpre, 7, 1, R, T, lens, want_data=ctx.needs_input_grad[1])
        g_mel = None
        if dxm is not None:
            B, _, Tm = ctx.mel_shape
            g_mel = empty(B, N_MEL, Tm)
            check(lib.radmmm_unsqueeze_rows(ptr(dxm), ptr(g_mel), B, N_MEL, Tm, 1, N_MEL, 0, s), "unsqueeze_rows")
        out = []
        for n, name in enumerate(names):
            gw, gb = grads[name]
            out += [gw if ctx.needs_input_grad[3 + 2 * n] else None, gb if ctx.needs_input_grad[4 + 2 * n] else None]
        return (None, g_mel, None, *out)


class Denoiser(nn.Module):
    """Denoiser(generator, filter_length=1024, n_overlap=4, win_length=1024, mode='zeros') of
    vocoders/hifigan_denoiser.py:25-58 on the GPU.  The bias spectrum (first STFT frame of the generator's output for a
    zero mel (1, 80, 88)) is computed with the HIP generator at the first call.

    forward(audio [B, S], strength=0.1, lens=None) -> [B, 1, (S // hop) * hop]; lens in samples (host or device), item
    b comes back with (lens[b] // hop) * hop samples and zeros beyond.  The reference reflect-pads by filter_length/2,
    which needs lens[b] > filter_length/2: shorter items raise."""

    def __init__(self, generator: HiFiGANGenerator, filter_length=1024, n_overlap=4, win_length=1024, mode="zeros"):
        super().__init__()
        if mode != "zeros":
            raise ValueError(f"Denoiser mode {mode!r} is not supported (only 'zeros')")
        self.__dict__["generator"] = generator          # not a sub-module: the reference's state_dict has no such keys
        self.filter_length = int(filter_length)
        self.hop_length = int(filter_length / n_overlap)
        self.win_length = int(win_length)
        n_fft, hop = self.filter_length, self.hop_length
        if n_fft % 4 or hop % 4 or (n_fft // 2) % hop or win_length != n_fft:
            raise ValueError("Denoiser: needs filter_length % 4 == 0, hop % 4 == 0, (filter_length/2) % hop == 0 and "
                             "win_length == filter_length")
        self.cutoff = n_fft // 2 + 1
        self.ldk = ops.round_up(2 * self.cutoff, 4)
        fb = np.fft.fft(np.eye(n_fft))
        fourier = np.vstack([np.real(fb[:self.cutoff]), np.imag(fb[:self.cutoff])])
        win = torch.from_numpy(_hann_periodic(win_length)).float()
        inv_basis = torch.from_numpy(np.linalg.pinv((n_fft / hop) * fourier).T).float() * win     # [2 cutoff, n_fft]
        self.register_buffer("forward_basis", torch.from_numpy(windowed_dft_basis(n_fft, win_length)))
        self.register_buffer("inverse_packed", pack_polyphase(inv_basis[:, None, :], hop, 0, (n_fft // 2) // hop,
                                                              self.ldk).contiguous())
        self.register_buffer("winsq", torch.from_numpy(_hann_periodic(win_length) ** 2))
        self.bias_spec = None

    def _bias(self, dev):
        if self.bias_spec is None or self.bias_spec.device != dev:
            mel0 = torch.zeros(1, N_MEL, 88, device=dev)
            audio = self.generator(mel0, precision="fp32")[:, 0]       # always the fp32 path, once per model
            spec = self._spectrum(audio, None, torch.ones(1, dtype=torch.int32, device=dev), 1)
            mag = torch.empty(self.cutoff, device=dev, dtype=torch.float32)
            check(lib.radmmm_voc_spec_bins(ptr(spec), self.ldk, 1, self.cutoff, None, 0.0, ptr(mag), stream()),
                  "voc_spec_bins")
            self.bias_spec = mag
        return self.bias_spec

    def _spectrum(self, audio, lens_d, frames_d, F):
        """windowed DFT of the reflect-padded frames: spec [B*F, ldk] (re | im), frames past frames_d[b] are 0"""
        B, S = audio.shape
        n_fft, hop = self.filter_length, self.hop_length
        pitch = ops.round_up(S + n_fft, 4)
        xpad = torch.empty(B * pitch, device=audio.device, dtype=torch.float32)
        check(lib.radmmm_voc_reflect_pad(ptr(audio), S, ptr(lens_d), ptr(xpad), B, S, n_fft // 2, pitch, stream()),
              "voc_reflect_pad")
        spec = torch.empty(B * F, self.ldk, device=audio.device, dtype=torch.float32)
        fb = self.forward_basis
        rowgemm(A=xpad, lda=hop, a_item_stride=pitch, B=fb, ldb=n_fft, b_tap_stride=0, C=spec, ldc=self.ldk, M=B * F,
                N=2 * self.cutoff, K=n_fft, taps=1, T=F, lens=frames_d, a_mask_mode=1, postmask=1)
        return spec

    @fp32_region
    def forward(self, audio: torch.Tensor, strength: float = 0.1, lens=None) -> torch.Tensor:
        if not audio.is_cuda:
            raise RadmmmError("Denoiser needs a GPU tensor (there is no CPU path)")
        if audio.dim() == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        audio = f32c(audio)
        B, S = audio.shape
        n_fft, hop = self.filter_length, self.hop_length
        dev = audio.device
        if S <= n_fft // 2:
            raise ValueError(f"Denoiser: {S} samples cannot be reflect-padded by {n_fft // 2} (needs > {n_fft // 2})")
        lens_d, host = _lens_arg(lens, B, S, dev)
        if host is not None:
            short = [int(v) for v in host if int(v) <= n_fft // 2]
            if short:
                raise ValueError(f"Denoiser: items of {short} samples cannot be reflect-padded by {n_fft // 2} "
                                 f"(the reference's reflect pad needs more than {n_fft // 2} samples: >= 3 mel frames)")
        elif bool((lens_d <= n_fft // 2).any()):       # device lengths: one synchronisation to validate them
            raise ValueError(f"Denoiser: every item needs more than {n_fft // 2} samples (>= 3 mel frames)")
        bias = self._bias(dev)
        F = 1 + S // hop
        frames_d = (_to_device(host // hop + 1, dev) if host is not None else lens_d // hop + 1).to(torch.int32)
        spec = self._spectrum(audio, lens_d, frames_d, F)
        check(lib.radmmm_voc_spec_bins(ptr(spec), self.ldk, B * F, self.cutoff, ptr(bias), float(strength), None,
                                       stream()), "voc_spec_bins")
        G = F - 1
        Wi = self.inverse_packed
        y = torch.empty(B, G * hop, device=dev, dtype=torch.float32)
        rowgemm(A=spec, lda=self.ldk, a_item_stride=F * self.ldk, B=Wi, ldb=self.ldk, b_tap_stride=Wi.stride(0), C=y,
                ldc=hop, M=B * G, N=hop, K=2 * self.cutoff, taps=Wi.shape[0], dil=1, T=G, lens=frames_d, a_mask_mode=1)
        check(lib.radmmm_voc_istft_finish(ptr(y), B, G * hop, ptr(frames_d), ptr(self.winsq), n_fft, hop, stream()),
              "voc_istft_finish")
        return y.view(B, 1, G * hop)


@fp32_region
def vocode(generator: HiFiGANGenerator, denoiser: Optional[Denoiser], mels: torch.Tensor, out_lens,
           strength: float = 0.001, normalize: bool = True, precision: Optional[str] = None
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """mels [B, 80, T] (descaled, as the reference passes them) + lengths in frames -> (audio [B, T*hop] zero padded,
    sample lengths [B] int64 on the host when out_lens was on the host, else on the device).  get_audio_for_mels
    (vocoder_utils.py:35-48) for the whole batch: generator, denoiser at `strength`, and with normalize each item
    scaled by 1 / max|audio| over its own samples.  precision: as HiFiGANGenerator.forward (None: generator.precision)."""
    mode = generator._mode(precision)
    if not mels.is_cuda:
        raise RadmmmError("vocode needs GPU tensors (there is no CPU path)")
    B, _, T = mels.shape
    dev = mels.device
    lens_d, host = _lens_arg(out_lens, B, T, dev)
    hop = generator.hop
    audio = generator._run(f32c(mels), lens_d, precision=mode)[:, 0]
    s_lens = host * hop if host is not None else lens_d.long() * hop
    if denoiser is not None:
        audio = denoiser(audio, strength, s_lens)[:, 0]
    audio = audio.contiguous()
    if normalize:
        check(lib.radmmm_voc_normalize(ptr(audio), audio.shape[1], ptr(lens_d * hop if host is None else
                                                                         _to_device(s_lens, dev)),
                                       B, audio.shape[1], stream()), "voc_normalize")
    return audio, s_lens


def load_hifigan_vocoder(checkpoint_path: str, config_path: str, device: Union[str, torch.device] = "cuda",
                         precision: str = "fp32"):
    """load_hifigan_vocoder of vocoders/vocoder_utils.py:104-132: the config JSON + torch.load(path)['generator'];
    the Gaussian blur stays off unless the path names it ('blur'), which this package does not support (raises).
    Returns (generator, denoiser) on `device`, in eval mode.  precision: the generator's `precision` attribute."""
    HiFiGANGenerator._check_precision(precision)
    with open(config_path) as fh:
        h = json.load(fh)
    if "blur" in checkpoint_path:
        h.setdefault("gaussian_blur", {})["p_blurring"] = 0.5
    else:
        h.setdefault("gaussian_blur", {})["p_blurring"] = 0.0
    sd = torch.load(checkpoint_path, map_location="cpu")["generator"]
    gen = HiFiGANGenerator(h)
    gen.load_state_dict(sd)
    gen = gen.to(device).eval()
    gen.precision = precision
    den = Denoiser(gen).to(device).eval()
    return gen, den
