"""WaveGlow vocoder + its STFT denoiser, batched on the GPU: mel -> waveform (reference
vocoders/waveglow_for_LIMMITS23/glow.py:62-311, denoiser.py, tacotron2/stft.py, vocoders/vocoder_utils.py:49-58, 134-143).

The reference's `infer` takes one utterance, knows no lengths and draws its noise inside the call.  Here a batch
[B, n_mel, T] with per-item lengths goes through one launch sequence, the noise can be handed in, item b equals a call
with item b alone at T = lens[b] given the same noise columns, and everything past lens[b] * hop is exactly 0.

Layout: channels-last rows of GROUP steps.  Row r = b*Tg + g (Tg = T * hop / n_group) holds the n_group consecutive
samples g*n_group .. of item b, as the reference's unfold does, and every layer treats rows at or past lens[b] * hop /
n_group as zeros (the reference's convolutions zero-pad at an utterance's end).  The flow variable X is an [R, n_group]
array whose c live channels sit RIGHT aligned in columns [n_group - c, n_group): an early re-attachment
cat(sigma * z, audio) writes n_early_size columns in front of them and nothing moves, and the final X is the waveform.

The wide convolutions are radmmm_rowgemm_f32 launches (exact fp32 MFMA): the ConvTranspose1d(n_mel, n_mel, 1024,
stride 256) as ONE polyphase row GEMM (pack_polyphase; output row group g takes input frames g - 3 .. g, and writing
exactly `stride` samples per frame is the reference's trim of kernel - stride samples), cond_layer once per flow for all
layers, the 3-tap in_layers with dilation 2^i, the 1x1 res_skip layers.  Everything else (grouping the conditioning,
start, the gate on a conditioning slice, the residual / skip update, end + inverse coupling + inverse 1x1 mix, the
noise columns, un-grouping) is a kernel of csrc/waveglow.hip.

That is precision "fp32", the default.  With WaveGlow.precision "h3" or "f16" infer runs cond_layer, the in_layers and the
res_skip layers on radmmm_rowgemm_h3 instead (fp16 operands, fp32 accumulation; three split products or one), and
wg_start_split / wg_gate_split / wg_res_skip_split write those GEMMs' fp16 operands in the pass that computes the value
(WaveGlow._wn_split); everything else, and every other entry point of this module, stays as described here.

The other direction, audio -> latent (glow.py:207-249 WaveGlow.forward, :43-59 WaveGlowLoss), runs the same WN launches
on the untouched half: the audio enters the rows with all n_group columns live (wg_group_audio), each flow is the forward
1x1 mix (wg_mix_fwd), the WN, and the forward coupling with the row's sum of log_s (wg_end_coupling_fwd); an early
output is n_early_size columns that simply stop being live, so the final X IS z in the reference's channel order; the
likelihood's two ragged sums are wg_nll_parts.

Training (train.py:62-152 of that vocoder): in training mode nll_loss and forward come out of one autograd node
(_WaveGlowFn) whose backward walks the flows from last to first, runs one flow's WN again into per-layer buffers and
back-propagates through it with row GEMMs (b_layout 1), radmmm_wgrad_f32, radmmm_colsum and the wg_*_bwd kernels;
apply_weight_norm / remove_weight_norm switch between the reference's weight_g / weight_v parameters and the folded
form.  Eval mode records no graph and runs exactly the launches above.  With WaveGlow.train_precision "h3" the step runs
the three GEMM families of every pass on the f16 matrix cores instead (_wn_split for the forward and the recomputation,
_backward_chunk_h3: radmmm_rowgemm_h3 / radmmm_wgrad_rm on pairs that wg_coupling_bwd_split, wg_gate_bwd_split and the
GEMM epilogues write times a power-of-two gradient scale).
"""
from __future__ import annotations

import ctypes
import json
import math
import pickle
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import nn

from . import ops
from ._lib import RadmmmError, check, f32c, fp32_region, lib, ptr, rowgemm, rowgemm_h3, stream, wgrad
from .vocoder import Denoiser, _lens_arg, _to_device, fold_weight_norm, pack_polyphase

UPSAMPLE_KERNEL = 1024     # glow.py:183-186: hard-coded in the reference
HOP = 256
_A_OPERAND_BYTES = 2 ** 31 - 2 ** 16     # the row GEMM's 16-row fast path needs A operands below 2 GiB
_COND_BYTES = 8 << 30                    # cap of the per-flow conditioning buffer [rows, 2 * n_channels * n_layers]
_TRAIN_ACT_BYTES = 8 << 30               # cap of what the backward of one flow holds (see WaveGlow._train_chunk)
PRECISIONS = ("fp32", "h3", "f16")       # WaveGlow.precision: how infer runs the three WN GEMM families
TRAIN_PRECISIONS = ("fp32", "h3")        # WaveGlow.train_precision: how the training step runs them
_WGRAD_RM_ITEMS = 1024                   # radmmm_wgrad_rm: items per launch


def auto_grad_scale(n_samples: int) -> float:
    """the automatic gradient scale of train_precision "h3": the smallest power of two at or above the batch's padded
    sample count B * T * 256, computed on the host.  A per-sample-normalised loss (nll_loss, WaveGlowLoss) seeds the
    backward pass with z / (sigma^2 N), N <= n_samples, so the scaled seed is z / sigma^2 times 1 .. 2 at equal lengths:
    of order 1, with fp16's 16 octaves up to 65504 above it and 14 octaves of normals plus 10 of subnormals below
    (DESIGN 4.19)."""
    return float(2 ** max(0, (max(1, int(n_samples)) - 1).bit_length()))


class _WN(nn.Module):
    """parameter holder with the reference WN's names (glow.py:105-151), weight norm already folded"""

    def __init__(self, n_in_channels, n_mel_channels, n_layers, n_channels, kernel_size):
        super().__init__()
        if kernel_size % 2 != 1:
            raise ValueError(f"WN kernel_size {kernel_size}: only odd kernels keep the length")
        if n_channels % 4:
            raise ValueError(f"WN n_channels {n_channels} must be a multiple of 4")
        self.n_layers, self.n_channels, self.kernel_size = int(n_layers), int(n_channels), int(kernel_size)
        self.start = nn.Conv1d(n_in_channels, n_channels, 1)
        self.end = nn.Conv1d(n_channels, 2 * n_in_channels, 1)
        nn.init.zeros_(self.end.weight)
        nn.init.zeros_(self.end.bias)
        self.cond_layer = nn.Conv1d(n_mel_channels, 2 * n_channels * n_layers, 1)
        self.in_layers = nn.ModuleList()
        self.res_skip_layers = nn.ModuleList()
        for i in range(n_layers):
            d = 2 ** i
            self.in_layers.append(nn.Conv1d(n_channels, 2 * n_channels, kernel_size, dilation=d,
                                            padding=(kernel_size * d - d) // 2))
            self.res_skip_layers.append(nn.Conv1d(n_channels, 2 * n_channels if i < n_layers - 1 else n_channels, 1))


class _Invertible1x1Conv(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv1d(c, c, 1, bias=False)
        W = torch.linalg.qr(torch.randn(c, c))[0]
        if torch.det(W) < 0:
            W[:, 0] = -W[:, 0]
        self.conv.weight.data = W.reshape(c, c, 1).contiguous()


def fold_weight_norm_keys(state_dict: dict) -> dict:
    """<name>.weight_g / <name>.weight_v (torch.nn.utils.weight_norm) or <name>.parametrizations.weight.original0 /
    original1 (its parametrization form) -> <name>.weight; every other key unchanged"""
    out = {}
    for k, v in state_dict.items():
        if k.endswith(".weight_g") or k.endswith(".parametrizations.weight.original0"):
            continue
        if k.endswith(".weight_v"):
            base = k[:-len(".weight_v")]
            out[base + ".weight"] = fold_weight_norm(v.float(), state_dict[base + ".weight_g"].float())
        elif k.endswith(".parametrizations.weight.original1"):
            base = k[:-len(".parametrizations.weight.original1")]
            out[base + ".weight"] = fold_weight_norm(v.float(),
                                                     state_dict[base + ".parametrizations.weight.original0"].float())
        else:
            out[k] = v
    return out


def unfold_weight_norm_keys(state_dict: dict, prefixes) -> dict:
    """the inverse direction for a model with weight norm applied: for every conv named in `prefixes` the keys become
    <name>weight_g / <name>weight_v (a folded <name>weight gives g = the rows' norms, v = the weight; the parametrization
    form is renamed); every other key unchanged"""
    out = {}
    for k, v in state_dict.items():
        base = next((p for p in prefixes if k.startswith(p)), None)
        leaf = k[len(base):] if base else None
        if leaf == "weight":
            v = v.float()
            out[base + "weight_g"] = v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
            out[base + "weight_v"] = v
        elif leaf == "parametrizations.weight.original0":
            out[base + "weight_g"] = v
        elif leaf == "parametrizations.weight.original1":
            out[base + "weight_v"] = v
        else:
            out[k] = v
    return out


class WaveGlow(nn.Module):
    """WaveGlow(n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config) of glow.py:178-205.
    state_dict keys are those of a reference model after remove_weightnorm (upsample.weight / .bias,
    WN.{k}.start / in_layers.{i} / cond_layer / res_skip_layers.{i} / end .weight / .bias, convinv.{k}.conv.weight);
    load_state_dict also takes the weight-normed keys (.weight_g / .weight_v) and folds them.

    infer(mel [B, n_mel, T], lens=None, sigma=1.0, noise=None, precision=None) -> audio [B, T * 256], exactly 0 at and past
    lens[b] * 256.  lens: lengths in mel frames, a host list / CPU tensor (no device -> host synchronisation) or a
    device int32 tensor.

    noise: None (drawn on the device) or the tuple of the reference's draws in the reference's order, each in the
    reference's layout [B, channels, Tg] with Tg = T * 256 / n_group group steps:
        noise[0]    [B, n_remaining_channels, Tg]   the initial draw (glow.py:265-267)
        noise[1 + j] [B, n_early_size, Tg]          one per early re-attachment, taken while k runs DOWN from
                                                    n_flows - 1 (glow.py:285-290: at every k > 0 with k % n_early_every
                                                    == 0), so noise[1] belongs to the largest such k
    Column g of every draw belongs to samples g*n_group .. g*n_group + n_group - 1; columns at or past an item's length
    are ignored.  Item b alone at T = lens[b] with noise[:][b:b+1, :, :lens[b] * 256 / n_group] gives the same audio.

    precision ("fp32", the default, "h3" or "f16"; the attribute `precision`, or per call infer(..., precision=)): how
    the mel -> audio direction runs the three WN GEMM families cond_layer, in_layers and res_skip_layers.  "fp32": the
    exact fp32 MFMA.  The other two run them on the f16 matrix cores (radmmm_rowgemm_h3, fp32 accumulation) with every
    operand element x of these GEMMs stored as fp16 values of s * x, s a power of two per tensor class (ops.W_SCALE for
    weights, 1 for activations): "f16" takes hi = fp16(s x) alone, half-precision vocoding as the reference's
    inference.py --is_fp16 offers it; "h3" takes the pair hi, lo = fp16(s x - hi) and sums hi.hi + hi.lo + lo.hi, which
    keeps fp32-class accuracy.  Everything else stays fp32 in every mode: the upsample, start, the gate, the residual
    stream H (an fp32 master copy; only its GEMM-operand copy is 16-bit), the skip sum, end, the coupling, the inverse
    mix and the flow variable.  Both need n_channels % 32 == 0 and (n_mel_channels * n_group) % 32 == 0, the GEMM's
    K % 32.  analyze, nll_loss, forward and training ignore the mode.

    analyze(mel [B, n_mel, T], audio [B, T * 256], lens=None, sigma=1.0) -> dict, everything on the device:
        z          [B, n_group, Tg] fp32   the reference's layout (early outputs first), exactly 0 past each length
        log_s_sum  [B] float64             sum of every coupling's log_s over the item's valid group steps
        log_det_W  [n_flows] float64       log|det W_k|, per group step (not multiplied by the batch)
        n_groups   [B] int64               valid group steps, lens[b] * 256 / n_group
        nll        [B] float64             (sum z^2 / (2 sigma^2) - log_s_sum[b] - n_groups[b] * sum_k log_det_W[k])
                                           / (n_groups[b] * n_group): nats per sample of item b
        loss       [] float64              the same expression over the batch's sums and sum_b n_groups[b] * n_group
    forward((mel, audio)) -> (z, log_s_list, log_det_W_list) as glow.py:207-249 (full lengths; log_det_W_list[k] =
    B * Tg * log|det W_k|, glow.py:100) for WaveGlowLoss; noise_from_z(z) -> the tuple `noise` of infer, so that
    infer(mel, lens, sigma=1.0, noise=noise_from_z(z)) returns the analysed audio.

    Training (self.training and grad mode on; eval mode is untouched): nll_loss(mel, audio, lens=None, sigma=1.0) -> the
    `loss` of analyze as a scalar with a grad_fn, and forward((mel, audio)) -> the same tuple with a grad_fn; backward()
    fills .grad of every parameter through the HIP backward pass (no atomics: two identical steps give identical bits;
    with host lengths no device -> host synchronisation).  apply_weight_norm() / remove_weight_norm() switch start,
    in_layers, cond_layer and res_skip_layers between weight_g / weight_v (a reference training checkpoint's keys) and
    the folded weight; load_state_dict takes either form in either state.  torch.optim.Adam on parameters() is the
    reference's optimizer.  One GPU.

    train_precision ("fp32", the default, or "h3"; the attribute, or per call nll_loss(..., precision=)): how a training
    step runs cond_layer, the in_layers and the res_skip layers.  "h3" runs them on the f16 matrix cores with three split
    products in every pass -- forward, the backward's recomputation, data gradients (radmmm_rowgemm_h3 against transposed
    split weights) and weight gradients (radmmm_wgrad_rm) -- while every master array, start / end, the coupling, the
    mixes, the likelihood, the upsample and the bias sums stay fp32.  Gradients enter the fp16 pairs times grad_scale:
    None (auto_grad_scale: the power of two at or above the padded sample count B * T * 256, computed on the host; it
    assumes a per-sample-normalised loss such as nll_loss or WaveGlowLoss) or a power of two; .grad holds the true values.
    grad_saturated() reads (and clears) the device flag a clamped pair raises; nothing else waits for the device.  It
    needs what infer's "h3" needs and at least 32 group steps per padded item.  "f16" (one product) is not built.  Eval
    mode, no_grad and `precision` (infer's switch) are not affected by it, nor it by them.

    Deliberate differences from the reference's forward: log|det W| where torch.logdet is NaN for a negative
    determinant; with ragged lengths every sum and the normalisation run over an item's own valid samples (the
    reference knows no lengths; with equal lengths `loss` equals WaveGlowLoss); lengths are given in mel frames."""

    def __init__(self, n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config):
        super().__init__()
        if n_group % 2 or HOP % n_group:
            raise ValueError(f"n_group {n_group} must be even and divide the hop {HOP}")
        if n_group > 8:
            raise ValueError(f"n_group {n_group}: the coupling kernel holds at most 8 channels")
        if n_early_size % 2:
            raise ValueError(f"n_early_size {n_early_size} must be even")
        self.n_mel_channels, self.n_flows, self.n_group = int(n_mel_channels), int(n_flows), int(n_group)
        self.n_early_every, self.n_early_size = int(n_early_every), int(n_early_size)
        self.hop = HOP
        self.upsample = nn.ConvTranspose1d(n_mel_channels, n_mel_channels, UPSAMPLE_KERNEL, stride=HOP)
        self.WN = nn.ModuleList()
        self.convinv = nn.ModuleList()
        n_half, n_rem = n_group // 2, n_group
        for k in range(n_flows):
            if k % n_early_every == 0 and k > 0:
                n_half -= n_early_size // 2
                n_rem -= n_early_size
            if n_rem < 2:
                raise ValueError("n_early_size / n_early_every leave no channels for the last flows")
            self.convinv.append(_Invertible1x1Conv(n_rem))
            self.WN.append(_WN(n_half, n_mel_channels * n_group, **WN_config))
        self.n_remaining_channels = n_rem
        self.precision = "fp32"
        self.train_precision = "fp32"
        self.grad_scale = None             # train_precision "h3": None (auto_grad_scale) or a power of two
        self._sat_flag = None              # device int32 [1]: OR-ed by the split producers of an "h3" backward pass
        self._folded = None
        self._folded_key = None
        self._weight_normed = False
        self._train_chunk_items = None     # items per chunk of the training step (None: from the memory caps)
        self._train_events = None          # a dict here receives the training step's device events (see _run)

    @property
    def noise_shapes(self):
        """channel counts of the draws of `noise`, in order"""
        early = [k for k in reversed(range(self.n_flows)) if k % self.n_early_every == 0 and k > 0]
        return [self.n_remaining_channels] + [self.n_early_size] * len(early)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        self._folded = None
        if self._weight_normed:
            state_dict = unfold_weight_norm_keys(state_dict, [n + "." for n, _ in self._normed_convs()])
        else:
            state_dict = fold_weight_norm_keys(state_dict)
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    # ---- weight norm as trainable parameters (glow.py:105-151: start, in_layers, cond_layer, res_skip_layers) --------
    def _normed_convs(self):
        for k, wn in enumerate(self.WN):
            yield f"WN.{k}.start", wn.start
            for i, m in enumerate(wn.in_layers):
                yield f"WN.{k}.in_layers.{i}", m
            yield f"WN.{k}.cond_layer", wn.cond_layer
            for i, m in enumerate(wn.res_skip_layers):
                yield f"WN.{k}.res_skip_layers.{i}", m

    def apply_weight_norm(self) -> "WaveGlow":
        """every conv the reference weight-norms gets weight_g [Cout, 1, 1] (the rows' norms) and weight_v (the weight)
        in place of weight, with the reference's names: state_dict() then has a reference training checkpoint's keys.
        `end`, `upsample` and the 1x1 mixes stay plain."""
        if self._weight_normed:
            return self
        for _, m in self._normed_convs():
            w = m.weight.detach()
            g = w.reshape(w.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
            del m._parameters["weight"]
            m.register_parameter("weight_g", nn.Parameter(g.clone()))
            m.register_parameter("weight_v", nn.Parameter(w.clone()))
        self._weight_normed, self._folded = True, None
        return self

    def remove_weight_norm(self) -> "WaveGlow":
        """back to the folded form: weight = weight_g * weight_v / ||weight_v||"""
        if not self._weight_normed:
            return self
        for _, m in self._normed_convs():
            w = fold_weight_norm(m.weight_v.detach().float(), m.weight_g.detach().float())
            del m._parameters["weight_g"], m._parameters["weight_v"]
            m.register_parameter("weight", nn.Parameter(w))
        self._weight_normed, self._folded = False, None
        return self

    # ---- weights in the kernels' layout, folded once (again only when a parameter changed) -------------------------
    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    @staticmethod
    def _gemm_weight(w: torch.Tensor, ldk: Optional[int] = None) -> torch.Tensor:
        """Conv1d weight [Cout, Cin, taps] -> [taps, Cout, ldk] (radmmm_rowgemm_f32 layout 0), zero padded to ldk"""
        Cout, Cin, taps = w.shape
        ldk = ldk or Cin
        W = torch.zeros(taps, Cout, ldk, device=w.device, dtype=torch.float32)
        W[:, :, :Cin] = w.detach().float().permute(2, 0, 1)
        return W

    def _weight_names(self):
        """the folded-form parameter names, in the order of the autograd node's weight arguments"""
        names = ["upsample.weight", "upsample.bias"]
        L = self.WN[0].n_layers
        for k in range(self.n_flows):
            p = f"WN.{k}."
            convs = (["start", "cond_layer"] + [f"in_layers.{i}" for i in range(L)]
                     + [f"res_skip_layers.{i}" for i in range(L)] + ["end"])
            for n in convs:
                names += [p + n + ".weight", p + n + ".bias"]
            names.append(f"convinv.{k}.conv.weight")
        return names

    @staticmethod
    def _conv_weight(m: nn.Module) -> torch.Tensor:
        """the conv's weight, folded from weight_g / weight_v where weight norm is applied (plain torch ops: autograd
        carries a gradient of the folded weight on to g and v)"""
        if "weight_g" in m._parameters:
            return fold_weight_norm(m.weight_v.float(), m.weight_g.float())
        return m.weight

    def _weights(self):
        out = []
        for n in self._weight_names():
            mod, leaf = n.rsplit(".", 1)
            m = self.get_submodule(mod)
            out.append(self._conv_weight(m) if leaf == "weight" else m.bias)
        return out

    def _fold(self):
        key = self._key()
        if self._folded is not None and self._folded_key == key:
            return self._folded
        W = {n: t.detach() for n, t in zip(self._weight_names(), self._weights())}
        invs, logdets = [], []
        for k in range(self.n_flows):
            w = W[f"convinv.{k}.conv.weight"]
            W64 = w[:, :, 0].double().cpu()
            invs.append(torch.linalg.inv(W64).float().to(w.device).contiguous())
            logdets.append(float(torch.linalg.slogdet(W64)[1]))
        f = self._pack(W, invs, torch.tensor(logdets, dtype=torch.float64).to(self.upsample.weight.device))
        self._folded, self._folded_key = f, key
        return f

    def _pack(self, W: dict, invs, logdet: torch.Tensor) -> dict:
        """folded weights by name (fp32, reference layouts) + W_k^-1 per flow + log|det W_k| [n_flows] float64 -> the
        kernels' layouts"""
        n_mel, ng = self.n_mel_channels, self.n_group
        L = self.WN[0].n_layers
        ldm = ops.round_up(n_mel, 4)
        f = {"ldm": ldm, "ldk": ops.round_up(n_mel * ng, 4)}
        f["up"] = (pack_polyphase(W["upsample.weight"].float(), HOP, 0, 0, ldm).contiguous(),
                   f32c(W["upsample.bias"]).repeat(HOP))
        flows = []
        for k in range(self.n_flows):
            p = f"WN.{k}."
            mix = W[f"convinv.{k}.conv.weight"]

            def wb(n, gemm=False, ldk=None):
                w = W[p + n + ".weight"]
                return (self._gemm_weight(w, ldk) if gemm else f32c(w[:, :, 0]), f32c(W[p + n + ".bias"]))
            flows.append({
                "c": mix.shape[0],
                "start": wb("start"),
                "cond": wb("cond_layer", True, f["ldk"]),
                "in": [wb(f"in_layers.{i}", True) for i in range(L)],
                "rs": [wb(f"res_skip_layers.{i}", True) for i in range(L)],
                "end": wb("end"),
                "inv": invs[k],
                "mix": f32c(mix[:, :, 0]),
            })
        f["flows"] = flows
        f["logdet"] = logdet
        return f

    def _noise_arg(self, noise, B: int, Tg: int, dev) -> Optional[list]:
        if noise is None:
            return None
        shapes = self.noise_shapes
        if len(noise) != len(shapes):
            raise ValueError(f"noise must hold {len(shapes)} draws (channels {shapes}), got {len(noise)}")
        out = []
        for z, ch in zip(noise, shapes):
            if tuple(z.shape) != (B, ch, Tg):
                raise ValueError(f"noise draw of shape {tuple(z.shape)}, expected {(B, ch, Tg)}")
            out.append(f32c(z.to(dev)))
        return out

    def _check_f16_gemm_k(self, what: str) -> None:
        """the shapes a 16-bit mode needs: K % 32 of the three GEMM families; `what` names the mode in the message"""
        C, K = self.WN[0].n_channels, self.n_mel_channels * self.n_group
        if C % 32 or K % 32:
            raise ValueError(f"{what} needs n_channels % 32 == 0 and (n_mel_channels * n_group) % 32 == 0 "
                             f"(the f16 GEMM's K % 32 == 0); got n_channels {C}, n_mel_channels * n_group {K}")

    def _precision(self, precision: Optional[str] = None) -> str:
        """the mode of a call (None: the attribute), checked: a known name, and for the 16-bit modes the GEMM's K % 32"""
        mode = self.precision if precision is None else precision
        if mode not in PRECISIONS:
            raise ValueError(f"precision {mode!r}: one of {PRECISIONS}")
        if mode != "fp32":
            self._check_f16_gemm_k(f"precision {mode!r}")
        return mode

    def _train_precision(self, precision: Optional[str] = None, mel: Optional[torch.Tensor] = None) -> str:
        """the mode of a training step (None: the attribute), checked like _precision: a known name, and for "h3" the
        GEMM's K % 32, a valid grad_scale and, given the batch, radmmm_wgrad_rm's T >= 32 group steps per padded item
        (the mode keeps no fp32 copy of its operands to fall back on)"""
        mode = self.train_precision if precision is None else precision
        if mode not in TRAIN_PRECISIONS:
            raise ValueError(f"train_precision {mode!r}: one of {TRAIN_PRECISIONS}"
                             + (" (one-product \"f16\" training is not built)" if mode == "f16" else ""))
        if mode == "h3":
            self._check_f16_gemm_k("train_precision 'h3'")
            self._g_scale(1)
            if mel is not None and mel.dim() == 3:
                Tg = mel.shape[2] * (HOP // self.n_group)
                if Tg < 32:
                    raise ValueError(f"train_precision 'h3' needs at least 32 group steps per padded item (the weight "
                                     f"gradient's K step); got {Tg}")
        return mode

    def _g_scale(self, n_samples: int) -> float:
        """the gradient scale of an "h3" step over n_samples = B * T * 256 padded samples"""
        if self.grad_scale is None:
            return auto_grad_scale(n_samples)
        g = float(self.grad_scale)
        if not (g > 0.0 and math.isfinite(g) and math.frexp(g)[0] == 0.5):
            raise ValueError(f"grad_scale {self.grad_scale!r} (train_precision 'h3'): None or a power of two")
        return g

    def grad_saturated(self) -> bool:
        """True when a split producer of an "h3" backward pass clamped a scaled gradient at fp16's range since the last
        call (the device flag word is read here and cleared: the only place that waits for the device).  Then lower
        grad_scale; the fp32 gradient arrays never carry the scale."""
        if self._sat_flag is None:
            return False
        hit = bool(int(self._sat_flag.item()) & 1)
        self._sat_flag.zero_()
        return hit

    def saturation_flag(self) -> torch.Tensor:
        """the device int32 [1] word grad_saturated() reads (created zeroed when no "h3" step has run yet), for a guard that
        stays on the device: `FlatAdam.step(skip=model.saturation_flag())` turns a clamped step into a no-op without a
        device -> host read.  Clearing it stays with grad_saturated()."""
        dev = next(self.parameters()).device
        if self._sat_flag is None or self._sat_flag.device != dev:
            self._sat_flag = torch.zeros(1, device=dev, dtype=torch.int32)
        return self._sat_flag

    @fp32_region
    def infer(self, mel: torch.Tensor, lens=None, sigma: float = 1.0, noise: Optional[Sequence[torch.Tensor]] = None,
              precision: Optional[str] = None) -> torch.Tensor:
        mode = self._precision(precision)
        if not mel.is_cuda:
            raise RadmmmError("WaveGlow needs a GPU tensor (there is no CPU path)")
        if mel.dim() != 3 or mel.shape[1] != self.n_mel_channels:
            raise ValueError(f"mel must be [B, {self.n_mel_channels}, T], got {tuple(mel.shape)}")
        B, _, T = mel.shape
        lens_d, _ = _lens_arg(lens, B, T, mel.device)
        return self._run(f32c(mel), lens_d, float(sigma), noise, precision=mode)

    def _chunk_items(self, f, Tg: int) -> int:
        """items per chunk: every GEMM A operand stays below 2 GiB and the conditioning buffer below its cap (items
        are independent, so the chunking changes no value)"""
        wn = self.WN[0]
        rows_cap = min(_A_OPERAND_BYTES // (4 * max(f["ldk"], wn.n_channels)),
                       _COND_BYTES // (8 * wn.n_channels * wn.n_layers))
        return max(1, rows_cap // Tg)

    def _run(self, mel: torch.Tensor, lens_d: torch.Tensor, sigma: float, noise=None,
             events: Optional[dict] = None, precision: Optional[str] = None) -> torch.Tensor:
        """mel [B, n_mel, T] fp32 on the device, lens_d int32 [B] on the device (frames).  Items are processed in chunks
        that keep every GEMM operand below 2 GiB (items are independent, so the chunking changes no value).
        events: a dict that receives (start, end) device events per launch family of the LAST chunk, and its row count
        under "rows" (timing).  precision: as infer."""
        mode = self._precision(precision)
        B, _, T = mel.shape
        dev = mel.device
        per = HOP // self.n_group
        Tg = T * per
        noise = self._noise_arg(noise, B, Tg, dev)
        f = self._fold()
        Bc = self._chunk_items(f, Tg)
        audio = torch.empty(B, T * HOP, device=dev, dtype=torch.float32)
        for b0 in range(0, B, Bc):
            b1 = min(B, b0 + Bc)
            self._run_chunk(f, mel[b0:b1], lens_d[b0:b1], sigma, None if noise is None else [z[b0:b1] for z in noise],
                            audio[b0:b1], events if b1 == B else None, mode)
        return audio

    @staticmethod
    def _timer(events: Optional[dict], R: int):
        if events is not None:
            events["rows"] = R

        def timed(name):
            if events is None:
                return lambda: None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            events.setdefault(name, []).append((e0, e1))
            e0.record()
            return e1.record
        return timed

    def _conditioning(self, f, mel, lens_d, lens_g, timed, keep_xm: bool = False):
        """upsample: one polyphase row GEMM over the mel frames, [B*T, HOP*n_mel] = channels-last [B*T*HOP, n_mel],
        then grouped into the conditioning rows [R, ldk]"""
        B, n_mel, T = mel.shape
        dev = mel.device
        ng = self.n_group
        Tg = T * (HOP // ng)
        s = stream()
        done = timed("upsample")
        ldm, ldk = f["ldm"], f["ldk"]
        xm = (torch.empty if ldm == n_mel else torch.zeros)(B * T, ldm, device=dev, dtype=torch.float32)
        check(lib.radmmm_squeeze_rows(ptr(mel), ptr(xm), B, n_mel, T, 1, ldm, 0, s), "squeeze_rows")
        Wp, bp = f["up"]
        up = torch.empty(B * T, HOP * n_mel, device=dev, dtype=torch.float32)
        rowgemm(A=xm, lda=ldm, B=Wp, ldb=Wp.shape[2], b_tap_stride=Wp.stride(0), C=up, ldc=HOP * n_mel, M=B * T,
                N=HOP * n_mel, K=n_mel, taps=Wp.shape[0], dil=1, T=T, lens=lens_d, a_mask_mode=1, bias=bp, postmask=1)
        ci = torch.empty(B * Tg, ldk, device=dev, dtype=torch.float32)
        check(lib.radmmm_wg_group_cond(ptr(up), T * HOP * n_mel, ptr(ci), ldk, ptr(lens_g), B, Tg, n_mel, ng, s),
              "wg_group_cond")
        done()
        if keep_xm:                     # the training step: the masked mel rows are the upsample's weight-gradient operand
            return ci, xm
        del up, xm
        return ci

    def _wn_buffers(self, R: int, dev):
        wn0 = self.WN[0]
        C, L = wn0.n_channels, wn0.n_layers

        def empty(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)
        return {"cond": empty(R, 2 * C * L), "H": empty(R, C), "S": empty(R, C), "acts": empty(R, C),
                "A": empty(R, 2 * C), "rs": empty(R, 2 * C)}

    def _wn(self, f, fk, X, col0: int, nh: int, ci, bufs, lens_g, R: int, Tg: int, timed) -> torch.Tensor:
        """the WN of one flow on the untouched half X[:, col0 : col0 + nh], the same launches in both directions: start,
        cond_layer for all layers, then per layer the dilated in_layer GEMM, the gate, the res_skip GEMM and the
        residual / skip update.  Returns the skip sum S [R, C], the input of `end`.  With bufs["layers"] (the training
        step's recomputation) layer i's input H_i, in_layer output A_i and gated acts_i stay in buffers of their own:
        one copy of H per layer more, the same values."""
        wn0 = self.WN[0]
        C, L, ksz = wn0.n_channels, wn0.n_layers, wn0.kernel_size
        ng, ldk = self.n_group, f["ldk"]
        cond, H, S, acts, A, rs = (bufs[n] for n in ("cond", "H", "S", "acts", "A", "rs"))
        layers = bufs.get("layers")
        if layers is not None:
            H = layers[0]["H"]
        s = stream()
        Ws, bs = fk["start"]
        done = timed("start")
        check(lib.radmmm_wg_start(ptr(X), ng, col0, nh, ptr(Ws), ptr(bs), ptr(H), C, C, ptr(lens_g), R, Tg, s),
              "wg_start")
        done()
        Wc, bc = fk["cond"]
        done = timed("cond_layer")
        rowgemm(A=ci, lda=ldk, B=Wc, ldb=ldk, b_tap_stride=0, C=cond, ldc=2 * C * L, M=R, N=2 * C * L,
                K=self.n_mel_channels * ng, taps=1, T=Tg, lens=lens_g, bias=bc)
        done()
        for i in range(L):
            if layers is not None:
                A, acts = layers[i]["A"], layers[i]["acts"]
            Wi, bi = fk["in"][i]
            done = timed("in_layers")
            rowgemm(A=H, lda=C, B=Wi, ldb=C, b_tap_stride=Wi.stride(0), C=A, ldc=2 * C, M=R, N=2 * C, K=C, taps=ksz,
                    dil=2 ** i, T=Tg, lens=lens_g, a_mask_mode=1, bias=bi)
            done()
            done = timed("gate")
            check(lib.radmmm_wg_gate(ptr(A), 2 * C, ptr(cond), 2 * C * L, 2 * C * i, ptr(acts), C, C, ptr(lens_g), R,
                                     Tg, s), "wg_gate")
            done()
            last = i == L - 1
            Wr, br = fk["rs"][i]
            done = timed("res_skip_gemm")
            rowgemm(A=acts, lda=C, B=Wr, ldb=C, b_tap_stride=0, C=rs, ldc=2 * C, M=R, N=C if last else 2 * C, K=C,
                    taps=1, T=Tg, lens=lens_g, bias=br)
            done()
            done = timed("res_skip_update")
            if layers is not None and not last:
                H = layers[i + 1]["H"].copy_(H)
            check(lib.radmmm_wg_res_skip(ptr(rs), 2 * C, ptr(H), C, ptr(S), C, C, int(i == 0), int(last),
                                         ptr(lens_g), R, Tg, s), "wg_res_skip")
            done()
        return S

    # ---- the 16-bit GEMM modes of infer ("h3" / "f16") -----------------------------------------------------------------
    @staticmethod
    def _split_weights(f, mode: str) -> list:
        """per flow the fp16 operands of the three GEMM families: the packed fp32 weights [taps, Cout, K] times
        ops.W_SCALE as the pair (hi, lo) for "h3", hi alone (lo None) for "f16".  Split once per fold and mode and kept
        inside the fold `f`, so they are dropped with it."""
        cache = f.setdefault("split", {})
        if mode not in cache:
            def sp(W):
                taps, Cout, K = W.shape
                hi, lo = ops.split_f16(W.view(taps * Cout, K), K, ops.W_SCALE, K, ops.NPROD[mode])
                return hi.view(taps, Cout, K), (lo.view(taps, Cout, K) if mode == "h3" else None)
            cache[mode] = [{"cond": sp(fk["cond"][0]), "in": [sp(W) for W, _ in fk["in"]],
                            "rs": [sp(W) for W, _ in fk["rs"]]} for fk in f["flows"]]
        return cache[mode]

    @staticmethod
    def _split_weights_t(f) -> list:
        """per flow the transposed "h3" pairs [taps, K, Cout] of _split_weights: the K-contiguous B operands of the data
        gradients (radmmm_rowgemm_h3 has no b_layout 1).  Made once per step and kept inside `f` like the pairs they are
        made from.  One radmmm_split_f16 and one radmmm_transpose_f16_pair launch per tensor: 2 L + 1 tensors per flow,
        2 * 12 * 17 = 408 launches on the shipped config (radmmm_transpose_f16_pair_multi takes the 8-bit format only)."""
        if "split_t" not in f:
            def tp(W):
                Wh, Wl = W
                _, Cout, K = Wh.shape
                return ops.transpose_split(Wh, Wl, Cout, K, Cout)
            f["split_t"] = [{"cond": tp(sw["cond"]), "in": [tp(W) for W in sw["in"]], "rs": [tp(W) for W in sw["rs"]]}
                            for sw in WaveGlow._split_weights(f, "h3")]
        return f["split_t"]

    def _wn_split_buffers(self, R: int, dev, mode: str):
        wn0 = self.WN[0]
        C, L = wn0.n_channels, wn0.n_layers

        def empty(*shape, dtype=torch.float32):
            return torch.empty(*shape, device=dev, dtype=dtype)

        def half():
            return empty(R, C, dtype=torch.float16)
        lo = mode == "h3"
        return {"cond": empty(R, 2 * C * L), "H": empty(R, C), "S": empty(R, C), "A": empty(R, 2 * C),
                "rs": empty(R, 2 * C), "Hh": half(), "Hl": half() if lo else None, "acts_h": half(),
                "acts_l": half() if lo else None}

    def _wn_split(self, f, fk, sw, X, col0: int, nh: int, cih, cil, bufs, lens_g, R: int, Tg: int, timed,
                  mode: str) -> torch.Tensor:
        """_wn for infer's 16-bit modes: the three GEMM families on radmmm_rowgemm_h3 (nprod 3 for "h3", 1 for "f16"),
        their A operands written as split fp16 copies by the kernels that produce the values (wg_start_split,
        wg_gate_split, wg_res_skip_split; cih / cil: the split conditioning rows).  The GEMMs' outputs, H, S and
        everything outside this function stay fp32.  With "f16" no lo half exists: the GEMM gets the hi array for both
        pointers and reads only that."""
        wn0 = self.WN[0]
        C, L, ksz = wn0.n_channels, wn0.n_layers, wn0.kernel_size
        ng, ldk = self.n_group, f["ldk"]
        cond, H, S, A, rs = (bufs[n] for n in ("cond", "H", "S", "A", "rs"))
        Hh, Hl, ah, al = (bufs[n] for n in ("Hh", "Hl", "acts_h", "acts_l"))
        layers = bufs.get("layers")     # the training step's recomputation: per layer the pair of H_i, A_i, the pair of acts_i
        if layers is not None:
            Hh, Hl = layers[0]["Hh"], layers[0]["Hl"]
        npr = ops.NPROD[mode]
        inv_ws = 1.0 / ops.W_SCALE

        def gemm(Ah, Al, lda, W, **kw):
            Wh, Wl = W
            rowgemm_h3(Ah=Ah, Al=Al if Al is not None else Ah, lda_h=lda, Bh=Wh, Bl=Wl if Wl is not None else Wh,
                       ldb_h=Wh.shape[2], b_tap_stride_h=Wh.stride(0), acc_scale=inv_ws, nprod=npr, M=R, T=Tg,
                       lens=lens_g, **kw)
        s = stream()
        Ws, bs = fk["start"]
        done = timed("start")
        check(lib.radmmm_wg_start_split(ptr(X), ng, col0, nh, ptr(Ws), ptr(bs), ptr(H), C, ptr(Hh), ptr(Hl), C, C,
                                        ptr(lens_g), R, Tg, s), "wg_start_split")
        done()
        done = timed("cond_layer")
        # In row slices whose output [rows][2 C L] stays below 2 GiB: the GEMM's direct epilogue addresses its arrays with
        # 32-bit byte offsets and a larger launch falls back to the general one (measured at 307 200 rows x 4096 columns,
        # one-product mode: 11.7 ms per launch against 2.8 ms for its three slices).  A 1x1 conv without a
        # mask: no row needs another row or its item's length, so any row boundary will do.
        step = max(128, ((2 ** 31 - 1) // (8 * C * L) - 64) // 128 * 128)
        Wch, Wcl = sw["cond"]
        for r0 in range(0, R, step):
            r1 = min(R, r0 + step)
            rowgemm_h3(Ah=cih[r0:r1], Al=(cil if cil is not None else cih)[r0:r1], lda_h=ldk, Bh=Wch,
                       Bl=Wcl if Wcl is not None else Wch, ldb_h=ldk, acc_scale=inv_ws, nprod=npr, C=cond[r0:r1],
                       ldc=2 * C * L, M=r1 - r0, N=2 * C * L, K=self.n_mel_channels * ng, taps=1, T=r1 - r0,
                       bias=fk["cond"][1])
        done()
        for i in range(L):
            if layers is not None:
                A, ah, al = layers[i]["A"], layers[i]["acts_h"], layers[i]["acts_l"]
            done = timed("in_layers")
            gemm(Hh, Hl, C, sw["in"][i], C=A, ldc=2 * C, N=2 * C, K=C, taps=ksz, dil=2 ** i, a_mask_mode=1,
                 bias=fk["in"][i][1])
            done()
            done = timed("gate")
            check(lib.radmmm_wg_gate_split(ptr(A), 2 * C, ptr(cond), 2 * C * L, 2 * C * i, ptr(ah), ptr(al), C, C,
                                           ptr(lens_g), R, Tg, s), "wg_gate_split")
            done()
            last = i == L - 1
            done = timed("res_skip_gemm")
            gemm(ah, al, C, sw["rs"][i], C=rs, ldc=2 * C, N=C if last else 2 * C, K=C, taps=1, bias=fk["rs"][i][1])
            done()
            done = timed("res_skip_update")
            if layers is not None and not last:     # H_{i+1}'s pair goes to the next layer's buffers; fp32 H in place
                Hh, Hl = layers[i + 1]["Hh"], layers[i + 1]["Hl"]
            check(lib.radmmm_wg_res_skip_split(ptr(rs), 2 * C, ptr(H), C, ptr(S), C, ptr(Hh), ptr(Hl), C, C, int(i == 0),
                                               int(last), ptr(lens_g), R, Tg, s), "wg_res_skip_split")
            done()
        return S

    def _run_chunk(self, f, mel, lens_d, sigma, noise, audio, events, mode: str = "fp32") -> None:
        B, n_mel, T = mel.shape
        dev = mel.device
        ng = self.n_group
        per = HOP // ng
        Tg, R = T * per, B * T * per
        C = self.WN[0].n_channels
        lens_g = lens_d * per
        s = stream()
        timed = self._timer(events, R)
        ci = self._conditioning(f, mel, lens_d, lens_g, timed)

        X = torch.empty(R, ng, device=dev, dtype=torch.float32)
        c = self.n_remaining_channels
        zi = 0

        def attach(ch, col0):
            nonlocal zi
            z = noise[zi] if noise is not None else torch.randn(B, ch, Tg, device=dev, dtype=torch.float32)
            zi += 1
            check(lib.radmmm_wg_noise_rows(ptr(z), sigma, ptr(X), ng, col0, ch, ptr(lens_g), B, Tg, s), "wg_noise_rows")

        attach(c, ng - c)
        if mode == "fp32":
            bufs = self._wn_buffers(R, dev)
        else:
            sw = self._split_weights(f, mode)
            bufs = self._wn_split_buffers(R, dev, mode)
            done = timed("split_cond")      # the conditioning rows feed every flow's cond_layer GEMM: one split pass
            cih, cil = ops.split_f16(ci, f["ldk"], 1.0, f["ldk"], ops.NPROD[mode])
            done()
            del ci
            if mode == "f16":
                cil = None
        for k in reversed(range(self.n_flows)):
            fk = f["flows"][k]
            assert fk["c"] == c
            nh, col0 = c // 2, ng - c
            if mode == "fp32":
                S = self._wn(f, fk, X, col0, nh, ci, bufs, lens_g, R, Tg, timed)
            else:
                S = self._wn_split(f, fk, sw[k], X, col0, nh, cih, cil, bufs, lens_g, R, Tg, timed, mode)
            We, be = fk["end"]
            done = timed("end_coupling")
            check(lib.radmmm_wg_end_coupling(ptr(S), C, ptr(We), ptr(be), ptr(fk["inv"]), ptr(X), ng, col0, nh, C,
                                             ptr(lens_g), R, Tg, s), "wg_end_coupling")
            done()
            if k % self.n_early_every == 0 and k > 0:
                attach(self.n_early_size, col0 - self.n_early_size)
                c += self.n_early_size
        assert c == ng
        done = timed("ungroup")
        check(lib.radmmm_wg_ungroup(ptr(X), ng, 0, ng, ptr(audio), audio.stride(0), ptr(lens_g), B, Tg, s), "wg_ungroup")
        done()

    # ---- audio -> latent ---------------------------------------------------------------------------------------------
    def _args_fwd(self, mel, audio):
        if not (mel.is_cuda and audio.is_cuda):
            raise RadmmmError("WaveGlow needs GPU tensors (there is no CPU path)")
        if mel.dim() != 3 or mel.shape[1] != self.n_mel_channels:
            raise ValueError(f"mel must be [B, {self.n_mel_channels}, T], got {tuple(mel.shape)}")
        B, _, T = mel.shape
        if tuple(audio.shape) != (B, T * HOP):
            raise ValueError(f"audio must be [B, T * {HOP}] = {(B, T * HOP)}, got {tuple(audio.shape)}")
        return f32c(mel), f32c(audio)

    def _analyze_run(self, mel, audio, lens_d, want_log_s: bool = False, events: Optional[dict] = None, f=None,
                     snaps=None, Bc=None, mode: str = "fp32"):
        """mel [B, n_mel, T], audio [B, T*HOP] fp32 on the device, lens_d int32 [B] on the device (frames) ->
        (z rows [B*Tg, n_group], parts [B, 2] float64 = (sum z^2, sum log_s) per item, the per-flow log_s rows
        [B*Tg, n_half_k] or None).  Chunked over items as _run; events as there.  f: the packed weights (default: the
        cached fold); snaps [n_flows, B*Tg, n_group]: receives the rows as they enter each flow (the training step).
        mode "h3" (the training step under train_precision "h3"): the WN through _wn_split."""
        B, _, T = mel.shape
        dev = mel.device
        ng = self.n_group
        Tg = T * (HOP // ng)
        f = f or self._fold()
        Bc = Bc or self._chunk_items(f, Tg)
        X = torch.empty(B * Tg, ng, device=dev, dtype=torch.float32)
        ls = torch.empty(B * Tg, device=dev, dtype=torch.float32)
        parts = torch.empty(B, 2, device=dev, dtype=torch.float64)
        logs = None
        if want_log_s:
            logs = [torch.empty(B * Tg, fk["c"] // 2, device=dev, dtype=torch.float32) for fk in f["flows"]]
        for b0 in range(0, B, Bc):
            b1 = min(B, b0 + Bc)
            r0, r1 = b0 * Tg, b1 * Tg
            self._analyze_chunk(f, mel[b0:b1], audio[b0:b1], lens_d[b0:b1], X[r0:r1], ls[r0:r1], parts[b0:b1],
                                None if logs is None else [t[r0:r1] for t in logs], events if b1 == B else None,
                                None if snaps is None else snaps[:, r0:r1], mode)
        return X, parts, logs

    def _analyze_chunk(self, f, mel, audio, lens_d, X, ls, parts, logs, events, snaps=None, mode: str = "fp32") -> None:
        B, _, T = mel.shape
        ng = self.n_group
        per = HOP // ng
        Tg, R = T * per, B * T * per
        C = self.WN[0].n_channels
        lens_g = lens_d * per
        s = stream()
        timed = self._timer(events, R)
        ci = self._conditioning(f, mel, lens_d, lens_g, timed)
        done = timed("group_audio")
        check(lib.radmmm_wg_group_audio(ptr(audio), audio.stride(0), ptr(X), ng, ng, ptr(lens_g), B, Tg, s),
              "wg_group_audio")
        done()
        if mode == "fp32":
            bufs = self._wn_buffers(R, mel.device)
        else:
            sw = self._split_weights(f, mode)
            bufs = self._wn_split_buffers(R, mel.device, mode)
            done = timed("split_cond")      # one split pass over the conditioning rows for every flow's cond_layer GEMM
            cih, cil = ops.split_f16(ci, f["ldk"], 1.0, f["ldk"], ops.NPROD[mode])
            done()
            del ci
        c = ng
        for k in range(self.n_flows):
            if k % self.n_early_every == 0 and k > 0:
                c -= self.n_early_size              # an early output: its columns stay where they are, as part of z
            fk = f["flows"][k]
            assert fk["c"] == c
            nh, col0 = c // 2, ng - c
            if snaps is not None:
                snaps[k].copy_(X)
            done = timed("mix_fwd")
            check(lib.radmmm_wg_mix_fwd(ptr(X), ng, col0, c, ptr(fk["mix"]), ptr(lens_g), R, Tg, s), "wg_mix_fwd")
            done()
            if mode == "fp32":
                S = self._wn(f, fk, X, col0, nh, ci, bufs, lens_g, R, Tg, timed)
            else:
                S = self._wn_split(f, fk, sw[k], X, col0, nh, cih, cil, bufs, lens_g, R, Tg, timed, mode)
            We, be = fk["end"]
            done = timed("end_coupling_fwd")
            check(lib.radmmm_wg_end_coupling_fwd(ptr(S), C, ptr(We), ptr(be), ptr(X), ng, col0, nh, C, ptr(ls),
                                                 int(k == 0), None if logs is None else ptr(logs[k]), ptr(lens_g), R,
                                                 Tg, s), "wg_end_coupling_fwd")
            done()
        assert c == self.n_remaining_channels
        done = timed("nll_parts")
        check(lib.radmmm_wg_nll_parts(ptr(X), ng, ng, ptr(ls), ptr(lens_g), B, Tg, ptr(parts), s), "wg_nll_parts")
        done()

    def _upsample_grads(self, f, dci, xm, lens_d, lens_g, B: int, T: int, out: dict) -> None:
        """the conditioning's gradient rows dci [R, ldk] -> channels-last gradient of the upsampled mel -> the polyphase
        GEMM's weight gradient against the masked mel rows xm, and the bias; into out (both training precisions: fp32)"""
        n_mel, ng = self.n_mel_channels, self.n_group
        Tg = T * (HOP // ng)
        dev = dci.device
        dup = torch.empty(B * T, HOP * n_mel, device=dev, dtype=torch.float32)
        check(lib.radmmm_wg_ungroup_cond(ptr(dci), f["ldk"], ptr(dup), T * HOP * n_mel, ptr(lens_g), B, Tg, n_mel, ng,
                                         stream()), "wg_ungroup_cond")
        taps = f["up"][0].shape[0]
        P = _wgrad(dup, HOP * n_mel, HOP * n_mel, xm, f["ldm"], n_mel, B * T, T, lens_d, taps, 1, 1)
        j = torch.arange(UPSAMPLE_KERNEL, device=dev)          # the inverse of pack_polyphase (padding 0, offset 0)
        out["upsample.weight"] = P.view(taps, HOP, n_mel, n_mel)[taps // 2 - j // HOP, j % HOP].permute(2, 1, 0)
        out["upsample.bias"] = _colsum(dup, HOP * n_mel, B * T, HOP * n_mel).view(HOP, n_mel).sum(0)

    def _backward_chunk(self, f, mel, lens_d, snaps, dX, g_ls, events) -> dict:
        """the backward pass of _analyze_chunk for the items of one chunk.  snaps [n_flows, R, n_group]: the rows as they
        entered each flow; dX [R, n_group]: the gradient of the final rows z on ALL columns (consumed: it becomes the
        gradient of the grouped audio, which nobody asks for); g_ls[k]: the gradient of flow k's log_s, one value [1] or
        rows [R, n_half_k].  Returns the gradients of the folded weights by name, reference layouts, WITHOUT the log-det
        terms of the mixes.  Every gradient row at or past an item's length is kept at 0."""
        B, n_mel, T = mel.shape
        dev = mel.device
        ng = self.n_group
        per = HOP // ng
        Tg, R = T * per, B * T * per
        wn0 = self.WN[0]
        C, L, ksz = wn0.n_channels, wn0.n_layers, wn0.kernel_size
        ldk, cols = f["ldk"], n_mel * ng
        lens_g = lens_d * per
        s = stream()
        timed = self._timer(events, R)
        ci, xm = self._conditioning(f, mel, lens_d, lens_g, timed, keep_xm=True)

        def empty(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)
        bufs = {"cond": empty(R, 2 * C * L), "S": empty(R, C), "rs": empty(R, 2 * C), "H": None, "A": None, "acts": None,
                "layers": [{"H": empty(R, C), "A": empty(R, 2 * C), "acts": empty(R, C)} for _ in range(L)]}
        dcond = empty(R, 2 * C * L)          # d cond; its column slice i is also d A_i, the GY of in_layer i
        GHS = empty(R, 2 * C)                # [d H_{i+1} | d S]: the A operand of the res_skip data gradient
        dacts, dO, Xp = empty(R, C), empty(R, ng), empty(R, ng)
        dci, dci_prev = empty(R, ldk), None
        out = {}
        for k in reversed(range(self.n_flows)):
            fk = f["flows"][k]
            c = fk["c"]
            nh, col0 = c // 2, ng - c
            p = f"WN.{k}."
            # recompute: the mixed rows and the WN on them, the launches (and bits) of the forward
            done = timed("bwd_recompute")
            Xp.copy_(snaps[k])
            check(lib.radmmm_wg_mix_fwd(ptr(Xp), ng, col0, c, ptr(fk["mix"]), ptr(lens_g), R, Tg, s), "wg_mix_fwd")
            S = self._wn(f, fk, Xp, col0, nh, ci, bufs, lens_g, R, Tg, lambda name: (lambda: None))
            done()
            We, be = fk["end"]
            done = timed("bwd_coupling")
            gl = g_ls[k]
            check(lib.radmmm_wg_coupling_bwd(ptr(S), C, ptr(We), ptr(be), ptr(Xp), ng, ptr(dX), ng, col0, nh, C, ptr(gl),
                                             0 if gl.dim() == 1 else nh, ptr(dO), ptr(GHS[:, C:]), 2 * C, ptr(lens_g), R,
                                             Tg, s), "wg_coupling_bwd")
            out[p + "end.weight"] = _outer_reduce(dO, 2 * nh, 2 * nh, S, C, C, lens_g, R, Tg)[:, :, None]
            out[p + "end.bias"] = _outer_reduce(None, 0, 1, dO, 2 * nh, 2 * nh, lens_g, R, Tg)[0]
            done()
            for i in reversed(range(L)):
                last = i == L - 1
                lay = bufs["layers"][i]
                Wi, _ = fk["in"][i]
                Wr, _ = fk["rs"][i]
                G, Mr = (GHS[:, C:], C) if last else (GHS, 2 * C)
                done = timed("bwd_res_skip")
                rowgemm(A=G, lda=2 * C, B=Wr, ldb=C, b_layout=1, C=dacts, ldc=C, M=R, N=C, K=Mr, T=Tg, lens=lens_g)
                out[p + f"res_skip_layers.{i}.weight"] = _wgrad(G, 2 * C, Mr, lay["acts"], C, C, R, Tg)[0][:, :, None]
                out[p + f"res_skip_layers.{i}.bias"] = _colsum(G, 2 * C, R, Mr)
                done()
                done = timed("bwd_gate")
                dA = dcond[:, 2 * C * i:]
                check(lib.radmmm_wg_gate_bwd(ptr(lay["A"]), 2 * C, ptr(bufs["cond"]), 2 * C * L, 2 * C * i, ptr(dacts), C,
                                             ptr(dA), 2 * C * L, C, ptr(lens_g), R, Tg, s), "wg_gate_bwd")
                done()
                done = timed("bwd_in_layers")
                out[p + f"in_layers.{i}.weight"] = _wgrad(dA, 2 * C * L, 2 * C, lay["H"], C, C, R, Tg, lens_g, ksz, 2 ** i,
                                                         1).permute(1, 2, 0)
                # d H_i = d H_{i+1} + the data gradient of the dilated conv (taps flipped: sign -1), in place in GHS
                rowgemm(A=dA, lda=2 * C * L, B=Wi, ldb=C, b_tap_stride=Wi.stride(0), b_layout=1, C=GHS, ldc=2 * C, M=R,
                        N=C, K=2 * C, taps=ksz, dil=2 ** i, sign=-1, T=Tg, lens=lens_g, a_mask_mode=0,
                        add=None if last else GHS, ldadd=2 * C, postmask=1)
                done()
            done = timed("bwd_start")
            Ws, _ = fk["start"]
            out[p + "start.weight"] = _outer_reduce(Xp[:, col0:], ng, nh, GHS, 2 * C, C, lens_g, R, Tg).t()[:, :, None]
            out[p + "start.bias"] = _outer_reduce(None, 0, 1, GHS, 2 * C, C, lens_g, R, Tg)[0]
            check(lib.radmmm_wg_start_bwd(ptr(GHS), 2 * C, ptr(Ws.t().contiguous()), ptr(dX), ng, col0, nh, C, ptr(lens_g),
                                          R, Tg, s), "wg_start_bwd")
            done()
            done = timed("bwd_cond_layer")
            Wc, _ = fk["cond"]
            bsum = _colsum(dcond, 2 * C * L, R, 2 * C * L)     # cond_layer's bias and, slice i, in_layer i's
            out[p + "cond_layer.bias"] = bsum
            for i in range(L):
                out[p + f"in_layers.{i}.bias"] = bsum[2 * C * i:2 * C * (i + 1)]
            out[p + "cond_layer.weight"] = _wgrad(dcond, 2 * C * L, 2 * C * L, ci, ldk, cols, R, Tg)[0][:, :, None]
            rowgemm(A=dcond, lda=2 * C * L, B=Wc, ldb=ldk, b_layout=1, C=dci, ldc=ldk, M=R, N=cols, K=2 * C * L, T=Tg,
                    lens=lens_g, add=dci_prev, ldadd=ldk)
            dci, dci_prev = (dci_prev if dci_prev is not None else empty(R, ldk)), dci
            done()
            done = timed("bwd_mix")
            out[f"convinv.{k}.conv.weight"] = _outer_reduce(dX[:, col0:], ng, c, snaps[k][:, col0:], ng, c, lens_g, R,
                                                            Tg)[:, :, None]
            check(lib.radmmm_wg_mix_fwd(ptr(dX), ng, col0, c, ptr(fk["mix"].t().contiguous()), ptr(lens_g), R, Tg, s),
                  "wg_mix_fwd")
            done()
        done = timed("bwd_upsample")
        self._upsample_grads(f, dci_prev, xm, lens_d, lens_g, B, T, out)
        done()
        return out

    def _backward_chunk_h3(self, f, mel, lens_d, snaps, dX, g_ls, events, g_scale: float) -> dict:
        """_backward_chunk under train_precision "h3": the data and weight gradients of cond_layer, the in_layers and the
        res_skip layers on the f16 matrix cores with three products (radmmm_rowgemm_h3 against the transposed split
        weights, radmmm_wgrad_rm on row-major pairs), the recomputation through _wn_split into per-layer pair buffers.
        Every fp32 array holds the true values, as in _backward_chunk; only the gradient pairs carry g_scale (written by
        wg_coupling_bwd_split, wg_gate_bwd_split and the in_layer data gradient's Ch / Cl), and acc_scale takes it and
        ops.W_SCALE out again.  start / end, the coupling, the mixes, every bias column sum and the upsample stay fp32."""
        B, n_mel, T = mel.shape
        dev = mel.device
        ng = self.n_group
        per = HOP // ng
        Tg, R = T * per, B * T * per
        wn0 = self.WN[0]
        C, L, ksz = wn0.n_channels, wn0.n_layers, wn0.kernel_size
        ldk, cols = f["ldk"], n_mel * ng
        lens_g = lens_d * per
        s = stream()
        timed = self._timer(events, R)
        if self._sat_flag is None or self._sat_flag.device != dev:
            self._sat_flag = torch.zeros(1, device=dev, dtype=torch.int32)
        flag = self._sat_flag
        sw, swt = self._split_weights(f, "h3"), self._split_weights_t(f)
        inv_g, inv_gw = 1.0 / g_scale, 1.0 / (g_scale * ops.W_SCALE)
        ci, xm = self._conditioning(f, mel, lens_d, lens_g, timed, keep_xm=True)
        done = timed("split_cond")
        cih, cil = ops.split_f16(ci, ldk, 1.0, ldk, 3)
        done()
        del ci

        def empty(*shape, dtype=torch.float32):
            return torch.empty(*shape, device=dev, dtype=dtype)

        def pair(n):
            return empty(R, n, dtype=torch.float16), empty(R, n, dtype=torch.float16)

        def wgrad_rm(gy, x, Mc, Nc, lens=None, taps=1, dil=1):
            P = ops.wgrad_rm_slabs(gy, x, B, Tg, Mc, Nc, taps, dil, inv_g, lens)
            return P.sum(0) if P.shape[0] > 1 else P[0]

        def layer():
            Hh, Hl = pair(C)
            ah, al = pair(C)
            return {"Hh": Hh, "Hl": Hl, "A": empty(R, 2 * C), "acts_h": ah, "acts_l": al}
        bufs = {"cond": empty(R, 2 * C * L), "H": empty(R, C), "S": empty(R, C), "rs": empty(R, 2 * C), "A": None,
                "Hh": None, "Hl": None, "acts_h": None, "acts_l": None, "layers": [layer() for _ in range(L)]}
        dcond = empty(R, 2 * C * L)          # d cond, fp32: the bias column sums read it
        dch, dcl = pair(2 * C * L)           # its scaled pair; column slice i is the GY / A operand of in_layer i
        GHS = empty(R, 2 * C)                # [d H_{i+1} | d S], fp32
        Gh, Gl = pair(2 * C)                 # its scaled pair: the A operand of the res_skip data gradient
        dacts, dO, Xp = empty(R, C), empty(R, ng), empty(R, ng)
        dci, dci_prev = empty(R, ldk), None
        out = {}
        for k in reversed(range(self.n_flows)):
            fk = f["flows"][k]
            c = fk["c"]
            nh, col0 = c // 2, ng - c
            p = f"WN.{k}."
            # recompute: the mixed rows and the WN on them, the launches (and bits) of this mode's forward
            done = timed("bwd_recompute")
            Xp.copy_(snaps[k])
            check(lib.radmmm_wg_mix_fwd(ptr(Xp), ng, col0, c, ptr(fk["mix"]), ptr(lens_g), R, Tg, s), "wg_mix_fwd")
            S = self._wn_split(f, fk, sw[k], Xp, col0, nh, cih, cil, bufs, lens_g, R, Tg, lambda name: (lambda: None),
                               "h3")
            done()
            We, be = fk["end"]
            done = timed("bwd_coupling")
            gl = g_ls[k]
            check(lib.radmmm_wg_coupling_bwd_split(ptr(S), C, ptr(We), ptr(be), ptr(Xp), ng, ptr(dX), ng, col0, nh, C,
                                                   ptr(gl), 0 if gl.dim() == 1 else nh, ptr(dO), ptr(GHS[:, C:]), 2 * C,
                                                   ptr(Gh[:, C:]), ptr(Gl[:, C:]), 2 * C, C, g_scale, ptr(flag),
                                                   ptr(lens_g), R, Tg, s), "wg_coupling_bwd_split")
            out[p + "end.weight"] = _outer_reduce(dO, 2 * nh, 2 * nh, S, C, C, lens_g, R, Tg)[:, :, None]
            out[p + "end.bias"] = _outer_reduce(None, 0, 1, dO, 2 * nh, 2 * nh, lens_g, R, Tg)[0]
            done()
            for i in reversed(range(L)):
                last = i == L - 1
                lay = bufs["layers"][i]
                G, Mr = (GHS[:, C:], C) if last else (GHS, 2 * C)
                Gp = (Gh[:, C:], Gl[:, C:]) if last else (Gh, Gl)
                done = timed("bwd_res_skip")
                Th, Tl = swt[k]["rs"][i]
                rowgemm_h3(Ah=Gp[0], Al=Gp[1], lda_h=2 * C, Bh=Th, Bl=Tl, ldb_h=Mr, acc_scale=inv_gw, nprod=3, C=dacts,
                           ldc=C, M=R, N=C, K=Mr, T=Tg, lens=lens_g)
                out[p + f"res_skip_layers.{i}.weight"] = wgrad_rm(Gp, (lay["acts_h"], lay["acts_l"]), Mr, C)[0][:, :, None]
                out[p + f"res_skip_layers.{i}.bias"] = _colsum(G, 2 * C, R, Mr)
                done()
                done = timed("bwd_gate")
                dA = dcond[:, 2 * C * i:]
                dAp = (dch[:, 2 * C * i:], dcl[:, 2 * C * i:])
                check(lib.radmmm_wg_gate_bwd_split(ptr(lay["A"]), 2 * C, ptr(bufs["cond"]), 2 * C * L, 2 * C * i,
                                                   ptr(dacts), C, ptr(dA), 2 * C * L, ptr(dAp[0]), ptr(dAp[1]), 2 * C * L,
                                                   2 * C, C, g_scale, ptr(flag), ptr(lens_g), R, Tg, s),
                      "wg_gate_bwd_split")
                done()
                done = timed("bwd_in_layers")
                out[p + f"in_layers.{i}.weight"] = wgrad_rm(dAp, (lay["Hh"], lay["Hl"]), 2 * C, C, lens_g, ksz,
                                                            2 ** i).permute(1, 2, 0)
                # d H_i = d H_{i+1} + the data gradient of the dilated conv (taps flipped: sign -1), fp32 in place in GHS
                # and as the scaled pair in the left half of the [dH | dS] pair
                Th, Tl = swt[k]["in"][i]
                rowgemm_h3(Ah=dAp[0], Al=dAp[1], lda_h=2 * C * L, Bh=Th, Bl=Tl, ldb_h=2 * C, b_tap_stride_h=Th.stride(0),
                           acc_scale=inv_gw, nprod=3, C=GHS, ldc=2 * C, M=R, N=C, K=2 * C, taps=ksz, dil=2 ** i, sign=-1,
                           T=Tg, lens=lens_g, a_mask_mode=0, add=None if last else GHS, ldadd=2 * C, postmask=1, Ch=Gh,
                           Cl=Gl, ldch=2 * C, ch_scale=g_scale, sat_flag=flag)
                done()
            done = timed("bwd_start")
            Ws, _ = fk["start"]
            out[p + "start.weight"] = _outer_reduce(Xp[:, col0:], ng, nh, GHS, 2 * C, C, lens_g, R, Tg).t()[:, :, None]
            out[p + "start.bias"] = _outer_reduce(None, 0, 1, GHS, 2 * C, C, lens_g, R, Tg)[0]
            check(lib.radmmm_wg_start_bwd(ptr(GHS), 2 * C, ptr(Ws.t().contiguous()), ptr(dX), ng, col0, nh, C, ptr(lens_g),
                                          R, Tg, s), "wg_start_bwd")
            done()
            done = timed("bwd_cond_layer")
            bsum = _colsum(dcond, 2 * C * L, R, 2 * C * L)     # cond_layer's bias and, slice i, in_layer i's
            out[p + "cond_layer.bias"] = bsum
            for i in range(L):
                out[p + f"in_layers.{i}.bias"] = bsum[2 * C * i:2 * C * (i + 1)]
            out[p + "cond_layer.weight"] = wgrad_rm((dch, dcl), (cih, cil), 2 * C * L, cols)[0][:, :, None]
            Th, Tl = swt[k]["cond"]
            rowgemm_h3(Ah=dch, Al=dcl, lda_h=2 * C * L, Bh=Th, Bl=Tl, ldb_h=2 * C * L, acc_scale=inv_gw, nprod=3, C=dci,
                       ldc=ldk, M=R, N=cols, K=2 * C * L, T=Tg, lens=lens_g, add=dci_prev, ldadd=ldk)
            dci, dci_prev = (dci_prev if dci_prev is not None else empty(R, ldk)), dci
            done()
            done = timed("bwd_mix")
            out[f"convinv.{k}.conv.weight"] = _outer_reduce(dX[:, col0:], ng, c, snaps[k][:, col0:], ng, c, lens_g, R,
                                                            Tg)[:, :, None]
            check(lib.radmmm_wg_mix_fwd(ptr(dX), ng, col0, c, ptr(fk["mix"].t().contiguous()), ptr(lens_g), R, Tg, s),
                  "wg_mix_fwd")
            done()
        done = timed("bwd_upsample")
        self._upsample_grads(f, dci_prev, xm, lens_d, lens_g, B, T, out)
        done()
        return out

    @fp32_region
    def analyze(self, mel: torch.Tensor, audio: torch.Tensor, lens=None, sigma: float = 1.0) -> dict:
        mel, audio = self._args_fwd(mel, audio)
        B, _, T = mel.shape
        ng = self.n_group
        Tg = T * (HOP // ng)
        lens_d, _ = _lens_arg(lens, B, T, mel.device)
        X, parts, _ = self._analyze_run(mel, audio, lens_d)
        logdet = self._fold()["logdet"]
        n_groups = lens_d.long() * (HOP // ng)
        sq, log_s_sum = parts[:, 0], parts[:, 1]
        num = sq / (2.0 * float(sigma) ** 2) - log_s_sum - n_groups * logdet.sum()
        return {"z": X.view(B, Tg, ng).transpose(1, 2).contiguous(), "log_s_sum": log_s_sum, "log_det_W": logdet,
                "n_groups": n_groups, "nll": num / (n_groups * ng), "loss": num.sum() / (n_groups.sum() * ng)}

    # ---- training: the same forward under one autograd node whose backward is the HIP path -------------------------
    def _train_active(self) -> bool:
        return self.training and torch.is_grad_enabled()

    @fp32_region
    def nll_loss(self, mel: torch.Tensor, audio: torch.Tensor, lens=None, sigma: float = 1.0,
                 precision: Optional[str] = None) -> torch.Tensor:
        """analyze(...)["loss"] as a scalar; in training mode with grad enabled it carries a grad_fn, and backward()
        fills .grad of every parameter (mel and audio get none).  With host lengths the step never waits for the
        device.  precision: the step's train_precision (None: the attribute); outside a training step the name is
        checked and the fp32 path runs."""
        if not self._train_active():
            if precision is not None:
                self._train_precision(precision)
            return self.analyze(mel, audio, lens, sigma)["loss"]
        mode = self._train_precision(precision, mel)
        mel, audio = self._args_fwd(mel, audio)
        lens_d, _ = _lens_arg(lens, mel.shape[0], mel.shape[2], mel.device)
        return _WaveGlowFn.apply(self, mel.detach(), audio.detach(), lens_d, float(sigma), True, mode, *self._weights())

    def _train_chunk(self, f, Tg: int, mode: str = "fp32") -> int:
        """items per chunk of a training step: the caps of _chunk_items, the conditioning gradient [rows, 2 C L] as a GEMM
        A operand, and _TRAIN_ACT_BYTES for what the backward of ONE flow holds per row (cond and its gradient, H_i / A_i /
        acts_i of every layer, the skip / res_skip / gradient rows, the conditioning rows and their two gradient copies).
        "h3": the fp16 pairs of H_i / acts_i / the conditioning rows take the bytes of the fp32 arrays they replace; the
        pairs of the conditioning gradient [rows, 2 C L] and of [dH | dS] and the one fp32 H come on top; every pair
        operand is half its fp32 twin's bytes, so the 2 GiB operand caps above cover radmmm_rowgemm_h3 and
        radmmm_wgrad_rm, whose 1024 items per launch cap the chunk as well."""
        if self._train_chunk_items:
            return int(self._train_chunk_items)
        wn = self.WN[0]
        C, L = wn.n_channels, wn.n_layers
        per_row = 4 * (8 * C * L + 8 * C + 3 * f["ldk"] + 3 * self.n_group + 8)
        if mode == "h3":
            per_row += 4 * (2 * C * L + 3 * C)
        rows_cap = min(_A_OPERAND_BYTES // (8 * C * L), _TRAIN_ACT_BYTES // per_row)
        items = max(1, min(self._chunk_items(f, Tg), rows_cap // Tg))
        return min(items, _WGRAD_RM_ITEMS) if mode == "h3" else items

    @fp32_region
    def forward(self, forward_input):
        mel, audio = forward_input
        mode = self._train_precision(None, mel) if self._train_active() else "fp32"
        mel, audio = self._args_fwd(mel, audio)
        if self._train_active():
            lens_d, _ = _lens_arg(None, mel.shape[0], mel.shape[2], mel.device)
            out = _WaveGlowFn.apply(self, mel.detach(), audio.detach(), lens_d, 1.0, False, mode, *self._weights())
            return out[0], list(out[1:-1]), list(out[-1].unbind(0))
        B, _, T = mel.shape
        ng = self.n_group
        Tg = T * (HOP // ng)
        lens_d, _ = _lens_arg(None, B, T, mel.device)
        X, _, logs = self._analyze_run(mel, audio, lens_d, want_log_s=True)
        logdet = self._fold()["logdet"]
        z = X.view(B, Tg, ng).transpose(1, 2).contiguous()
        log_s_list = [t.view(B, Tg, -1).transpose(1, 2).contiguous() for t in logs]
        return z, log_s_list, [logdet[k] * (B * Tg) for k in range(self.n_flows)]

    def noise_from_z(self, z: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """z [B, n_group, Tg] of analyze / forward -> the draws of infer's `noise`: the last n_remaining_channels
        channels, then the early blocks from the latest exit to the earliest"""
        if z.dim() != 3 or z.shape[1] != self.n_group:
            raise ValueError(f"z must be [B, {self.n_group}, Tg], got {tuple(z.shape)}")
        lo = self.n_group - self.n_remaining_channels
        out = [z[:, lo:]]
        while lo > 0:
            out.append(z[:, lo - self.n_early_size:lo])
            lo -= self.n_early_size
        return tuple(t.contiguous() for t in out)


def _outer_reduce(A, lda, M, Bm, ldb, N, lens_g, R, Tg) -> torch.Tensor:
    """out [M, N] = sum over the valid rows of A[r, :M]^T B[r, :N] (A None: column sums [1, N]); views into wider rows"""
    M = M if A is not None else 1
    out = torch.empty(M, N, device=Bm.device, dtype=torch.float32)
    scratch = torch.empty(int(lib.radmmm_wg_outer_reduce_scratch_floats(R, M, N)), device=Bm.device, dtype=torch.float32)
    check(lib.radmmm_wg_outer_reduce(ptr(A), lda, M, ptr(Bm), ldb, N, ptr(out), ptr(scratch), ptr(lens_g), R, Tg,
                                     stream()), "wg_outer_reduce")
    return out


def _colsum(X, ld, R, cols) -> torch.Tensor:
    out = torch.empty(cols, device=X.device, dtype=torch.float32)
    scratch = torch.empty(int(lib.radmmm_colsum_scratch_floats(R, cols)), device=X.device, dtype=torch.float32)
    check(lib.radmmm_colsum(ptr(X), ld, ptr(out), ptr(scratch), R, cols, 0, 1, None, 1, 1, 0, stream()), "colsum")
    return out


def _wgrad(GY, ldgy, Mc, X, ldx, Nc, R, T, lens=None, taps=1, dil=1, x_mask_mode=0) -> torch.Tensor:
    """[taps, Mc, Nc] = sum_r GY[r, :Mc]^T Xm[r + (tap - taps // 2) * dil, :Nc]: split-K slabs added in slab order"""
    S = ops.pick_splits(-(-Mc // 128) * -(-Nc // 128) * taps, R)
    P = torch.empty(S, taps, Mc, Nc, device=X.device, dtype=torch.float32)
    wgrad(GY=GY, ldgy=ldgy, X=X, ldx=ldx, P=P, ldp=Nc, split_stride=P.stride(0), R=R, Mc=Mc, Nc=Nc, taps=taps, dil=dil,
          T=T, lens=lens, x_mask_mode=x_mask_mode, splits=S)
    return P.sum(0) if S > 1 else P[0]


def inv_logdet(mixes) -> Tuple[list, torch.Tensor]:
    """[c_k, c_k] fp32 matrices on the device -> ([W_k^-1 fp32], log|det W_k| [n] float64) from one launch"""
    dev = mixes[0].device
    cs = [int(w.shape[0]) for w in mixes]
    Wp = torch.cat([f32c(w).reshape(-1) for w in mixes])
    Wi = torch.empty_like(Wp)
    logdet = torch.empty(len(cs), device=dev, dtype=torch.float64)
    check(lib.radmmm_wg_inv_logdet(ptr(Wp), (ctypes.c_int32 * len(cs))(*cs), len(cs), ptr(Wi), ptr(logdet), stream()),
          "wg_inv_logdet")
    offs = [0]
    for c in cs:
        offs.append(offs[-1] + c * c)
    return [Wi[offs[k]:offs[k + 1]].view(cs[k], cs[k]) for k in range(len(cs))], logdet


class _WaveGlowFn(torch.autograd.Function):
    """WaveGlow.forward / nll_loss as one autograd node.  Inputs: the module, mel, audio, lens (device int32, frames),
    sigma, fused, mode (the step's train_precision), then the folded weights in WaveGlow._weight_names() order (reference
    layouts).  fused: the output is the
    ragged loss of analyze(); else (z [B, n_group, Tg], log_s per flow [B, n_half_k, Tg], B * Tg * log|det W_k|
    [n_flows] float64).  The forward keeps the rows as they enter each flow (32 bytes per row and flow); the backward
    walks the flows from last to first, recomputes one flow's WN into per-layer buffers and back-propagates through it
    (DESIGN 4.19)."""

    @staticmethod
    def forward(ctx, model, mel, audio, lens_d, sigma, fused, mode, *weights):
        B, _, T = mel.shape
        ng = model.n_group
        per = HOP // ng
        Tg = T * per
        dev = mel.device
        W = dict(zip(model._weight_names(), weights))
        invs, logdet = inv_logdet([W[f"convinv.{k}.conv.weight"][:, :, 0] for k in range(model.n_flows)])
        f = model._pack(W, invs, logdet)
        Bc = model._train_chunk(f, Tg, mode)
        snaps = torch.empty(model.n_flows, B * Tg, ng, device=dev, dtype=torch.float32)
        X, parts, logs = model._analyze_run(mel, audio, lens_d, want_log_s=not fused, events=model._train_events, f=f,
                                             snaps=snaps, Bc=Bc, mode=mode)
        ctx.model, ctx.f, ctx.sigma, ctx.fused, ctx.Bc, ctx.mode = model, f, sigma, fused, Bc, mode
        if mode == "h3":          # a power of two from the padded sample count alone: no device value is read for it
            ctx.g_scale = model._g_scale(B * T * HOP)
        ctx.save_for_backward(mel, audio, lens_d, snaps, X)
        if fused:
            n_groups = lens_d.long() * per
            num = parts[:, 0] / (2.0 * sigma ** 2) - parts[:, 1] - n_groups * logdet.sum()
            return num.sum() / (n_groups.sum() * ng)
        z = X.view(B, Tg, ng).transpose(1, 2).contiguous()
        log_s = [t.view(B, Tg, -1).transpose(1, 2).contiguous() for t in logs]
        return (z, *log_s, logdet * (B * Tg))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        model, f, sigma = ctx.model, ctx.f, ctx.sigma
        mel, audio, lens_d, snaps, X = ctx.saved_tensors
        B, _, T = mel.shape
        ng = model.n_group
        per = HOP // ng
        Tg = T * per
        dev = mel.device
        nhs = [fk["c"] // 2 for fk in f["flows"]]
        if ctx.fused:
            # loss = (sum z^2 / (2 sigma^2) - sum log_s - sum_b n_b sum_k logdet_k) / N, N = sum_b n_b * n_group
            g = grads[0].double()
            N = (lens_d.long().sum() * (per * ng)).double()
            dX = X * (g / (sigma ** 2 * N)).float()
            g_ls = [(-g / N).float().reshape(1)] * model.n_flows
            g_logdet = (-g / ng).float().expand(model.n_flows)
        else:
            gz, gl = grads[0], grads[1:-1]
            dX = (torch.zeros_like(X) if gz is None
                  else gz.float().transpose(1, 2).reshape(B * Tg, ng).contiguous().clone())
            g_ls = [torch.zeros(B * Tg, nh, device=dev) if t is None
                    else t.float().transpose(1, 2).reshape(B * Tg, nh).contiguous() for t, nh in zip(gl, nhs)]
            g_logdet = (torch.zeros(model.n_flows, device=dev) if grads[-1] is None
                        else (grads[-1].double() * (B * Tg)).float())
        total = None
        for b0 in range(0, B, ctx.Bc):                 # a fixed order: the chunks' gradients are added as they come
            b1 = min(B, b0 + ctx.Bc)
            r0, r1 = b0 * Tg, b1 * Tg
            args = (f, mel[b0:b1], lens_d[b0:b1], snaps[:, r0:r1], dX[r0:r1],
                    [t if t.shape[0] == 1 else t[r0:r1] for t in g_ls], model._train_events if b1 == B else None)
            part = (model._backward_chunk(*args) if ctx.mode == "fp32"
                    else model._backward_chunk_h3(*args, g_scale=ctx.g_scale))
            total = part if total is None else {n: total[n] + part[n] for n in total}
        Wn = dict(zip(model._weight_names(), ctx.needs_input_grad[7:]))
        for k in range(model.n_flows):                 # the log-det terms: d log|det W| / dW = W^-T
            n = f"convinv.{k}.conv.weight"
            total[n] = total[n] + (g_logdet[k] * f["flows"][k]["inv"].t())[:, :, None]
        return (None,) * 7 + tuple(total[n] if need else None for n, need in Wn.items())


class WaveGlowLoss(nn.Module):
    """WaveGlowLoss(sigma) of glow.py:43-59 on the tuple WaveGlow.forward returns:
    (sum z^2 / (2 sigma^2) - sum log_s - sum log_det_W) / z.numel(), a few reductions in float64"""

    def __init__(self, sigma: float = 1.0):
        super().__init__()
        self.sigma = float(sigma)

    def forward(self, model_output):
        z, log_s_list, log_det_W_list = model_output
        log_s_total = sum(t.double().sum() for t in log_s_list)
        log_det_W_total = sum(t.double() for t in log_det_W_list)
        loss = (z.double() ** 2).sum() / (2.0 * self.sigma * self.sigma) - log_s_total - log_det_W_total
        return loss / z.numel()


class WaveGlowDenoiser(Denoiser):
    """Denoiser(waveglow, filter_length=1024, n_overlap=4, win_length=1024, mode='zeros') of
    vocoders/waveglow_for_LIMMITS23/denoiser.py on the GPU: the bias spectrum is the magnitude of frame 0 of the STFT of
    waveglow.infer(zeros(1, n_mel, 88), sigma=0), computed with the HIP path at the first call; forward is STFT ->
    clamp(mag - bias * strength, 0) -> inverse STFT with the original phase.  The reference's tacotron2/stft.py and the
    audio_processing.py the HiFi-GAN denoiser uses are the same transform (reflect pad, window-sum-square division,
    filter_length / 2 trimmed at both ends), so everything but the bias is vocoder.Denoiser's.

    The bias spectrum is always computed on the fp32 path, whatever waveglow.precision says (88 frames, once per model):
    one denoiser serves a model in every mode.

    forward(audio [B, S], strength=0.1, lens=None) -> [B, 1, (S // hop) * hop]; lens in samples."""

    def __init__(self, waveglow: WaveGlow, filter_length=1024, n_overlap=4, win_length=1024, mode="zeros"):
        super().__init__(waveglow, filter_length, n_overlap, win_length, mode)

    def _bias(self, dev):
        if self.bias_spec is None or self.bias_spec.device != dev:
            wg = self.generator
            audio = wg.infer(torch.zeros(1, wg.n_mel_channels, 88, device=dev), sigma=0.0, precision="fp32")
            spec = self._spectrum(audio, None, torch.ones(1, dtype=torch.int32, device=dev), 1)
            mag = torch.empty(self.cutoff, device=dev, dtype=torch.float32)
            check(lib.radmmm_voc_spec_bins(ptr(spec), self.ldk, 1, self.cutoff, None, 0.0, ptr(mag), stream()),
                  "voc_spec_bins")
            self.bias_spec = mag
        return self.bias_spec


@fp32_region
def vocode_waveglow(model: WaveGlow, denoiser: Optional[WaveGlowDenoiser], mels: torch.Tensor, out_lens,
                    sigma: float = 0.667, strength: float = 0.001, normalize: bool = True,
                    precision: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """mels [B, n_mel, T] + lengths in frames -> (audio [B, T*256] zero padded, sample lengths [B] int64 on the host
    when out_lens was on the host, else on the device).  The waveglow branch of get_audio_for_mels
    (vocoder_utils.py:49-58) for a whole batch: infer at `sigma`, denoiser at `strength`, and with normalize each item
    divided by max|audio| over its own samples.  precision: as WaveGlow.infer (None: model.precision)."""
    mode = model._precision(precision)
    if not mels.is_cuda:
        raise RadmmmError("vocode_waveglow needs GPU tensors (there is no CPU path)")
    B, _, T = mels.shape
    dev = mels.device
    lens_d, host = _lens_arg(out_lens, B, T, dev)
    audio = model._run(f32c(mels), lens_d, float(sigma), precision=mode)
    s_lens = host * HOP if host is not None else lens_d.long() * HOP
    if denoiser is not None:
        audio = denoiser(audio, strength, s_lens)[:, 0]
    audio = audio.contiguous()
    if normalize:
        sl = lens_d * HOP if host is None else _to_device(s_lens, dev)
        check(lib.radmmm_voc_normalize(ptr(audio), audio.shape[1], ptr(sl), B, audio.shape[1], stream()), "voc_normalize")
    return audio, s_lens


def config_of_module(m) -> dict:
    """the constructor arguments of an unpickled reference WaveGlow module, read from its attributes"""
    wn = m.WN[0]
    return {"n_mel_channels": int(m.upsample.weight.shape[0]), "n_flows": int(m.n_flows), "n_group": int(m.n_group),
            "n_early_every": int(m.n_early_every), "n_early_size": int(m.n_early_size),
            "WN_config": {"n_layers": int(wn.n_layers), "n_channels": int(wn.n_channels),
                          "kernel_size": int(wn.in_layers[0].kernel_size[0])}}


def load_waveglow_vocoder(checkpoint_path: str, config_path: Optional[str] = None,
                          device: Union[str, torch.device] = "cuda", allow_pickled_module: bool = False,
                          precision: str = "fp32"):
    """load_waveglow_vocoder of vocoders/vocoder_utils.py:134-143.  Two checkpoint formats:
      * a plain file {'state_dict': ..., 'waveglow_config': {...}} (see INTEGRATION.md for the one-line conversion);
        without 'waveglow_config' the config JSON's "waveglow_config" section is used;
      * the reference's own {'model': <pickled WaveGlow module>}: only with allow_pickled_module=True, because
        unpickling a module runs whatever code the file names (load such files from sources you trust only) and needs
        the reference's glow.py on sys.path (this package never imports it); its state_dict and attributes are
        copied out.
    The file is read with torch's restricted unpickler first; a file that this refuses is fully unpickled only when the
    caller opted in.  Returns (waveglow, denoiser) on `device`, in eval mode.  precision: the model's `precision`
    attribute ("fp32", "h3" or "f16", see WaveGlow); a mode the config cannot run raises ValueError here."""
    try:
        ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        if not allow_pickled_module:
            raise ValueError(f"{checkpoint_path} is not a plain {{'state_dict', 'waveglow_config'}} file ({e}); a "
                             "reference checkpoint holding a pickled module loads with allow_pickled_module=True, or "
                             "convert it once (INTEGRATION.md)") from e
        ck = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    if "state_dict" in ck:
        sd, cfg = ck["state_dict"], ck.get("waveglow_config")
    elif "model" in ck:
        sd, cfg = ck["model"].state_dict(), config_of_module(ck["model"])
    else:
        raise ValueError(f"{checkpoint_path}: neither 'state_dict' nor 'model' in the checkpoint")
    if cfg is None:
        if config_path is None:
            raise ValueError("load_waveglow_vocoder: the checkpoint carries no 'waveglow_config' and no config_path given")
        with open(config_path) as fh:
            cfg = json.load(fh)
        cfg = cfg.get("waveglow_config", cfg)
    model = WaveGlow(**cfg)
    model.precision = model._precision(precision)
    model.load_state_dict(sd)
    model = model.to(device).eval()
    den = WaveGlowDenoiser(model).to(device).eval()
    return model, den
