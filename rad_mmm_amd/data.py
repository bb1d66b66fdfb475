"""On-device pieces of the reference's data path (reference data.py).

The reference computes the attention prior and the energy average per utterance on CPU dataset
workers (scipy.stats.betabinom + scipy.ndimage.zoom; `mel.mean(0)`), caches priors on disk, and pads
them into the batch in DataCollate.  Here the same quantities come from libradmmm_hip.so
(csrc/prior.hip): anchor priors are built once per rounded size and kept on the device, a whole batch
is interpolated / renormalised / zero-padded in one launch.  Same names and argument meaning as
data.py; results are device tensors (fp32, as DataCollate's FloatTensor batch).  float64 arithmetic
inside, as scipy.  There is no CPU path.

DeviceCollate (csrc/collate.hip) puts the pieces together: raw items in -- samples, token ids, cached
pyin tracks --, the batch dictionary of DataCollate out, on the device; plan_batch is its host half."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import lib, check, ptr, stream, RadmmmError


def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RadmmmError("rad_mmm_amd.data needs a GPU (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def beta_binomial_prior_distribution(phoneme_count: int, mel_count: int, scaling_factor: float = 0.05,
                                     device=None) -> torch.Tensor:
    """data.py:90-102 -> float64 [mel_count, phoneme_count] on the device."""
    out = torch.empty(int(mel_count), int(phoneme_count), device=_device(device), dtype=torch.float64)
    check(lib.radmmm_betabinom_prior(int(phoneme_count), int(mel_count), float(scaling_factor), ptr(out), stream()),
          "betabinom_prior")
    return out


class BetaBinomialInterpolator:
    """data.py:61-88: anchor priors at sizes rounded to (round_mel_len_to, round_text_len_to), bilinear
    zoom (scipy.ndimage.zoom order=1 semantics) to the utterance's size, rows renormalised.  The bank
    (the reference's lru_cache) lives on the device."""

    def __init__(self, round_mel_len_to: int = 100, round_text_len_to: int = 20, scaling_factor: float = 0.05,
                 device=None):
        self.round_mel_len_to = round_mel_len_to
        self.round_text_len_to = round_text_len_to
        self.scaling_factor = scaling_factor
        self.device = _device(device)
        self._bank: Dict[Tuple[int, int], torch.Tensor] = {}

    @staticmethod
    def round(val, to):
        return max(1, int(round((val + 1) / to))) * to            # numpy.round: half to even, as Python's round

    def bank(self, bw: int, bh: int) -> torch.Tensor:
        t = self._bank.get((bw, bh))
        if t is None:
            t = self._bank[(bw, bh)] = beta_binomial_prior_distribution(bw, bh, self.scaling_factor, self.device)
        return t

    def batch(self, in_lens: Sequence[int], out_lens: Sequence[int]) -> torch.Tensor:
        """Padded [B, max(out_lens), max(in_lens)] fp32 prior of a batch (DataCollate, data.py:678-679,737-741);
        in_lens / out_lens are host integers (token and frame counts), as the dataset has them."""
        in_lens = [int(v) for v in in_lens]
        out_lens = [int(v) for v in out_lens]
        if len(in_lens) != len(out_lens) or not in_lens or min(in_lens) < 1 or min(out_lens) < 1:
            raise ValueError("in_lens / out_lens: same non-zero length, all counts >= 1")
        rows = []
        for p, m in zip(in_lens, out_lens):
            bh = self.round(m, self.round_mel_len_to)
            bw = self.round(p, self.round_text_len_to)
            rows.append([self.bank(bw, bh).data_ptr(), bh, bw, m, p])
        items = torch.tensor(rows, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)   # (no blocking copy)
        B, Tmax, Nmax = len(rows), max(out_lens), max(in_lens)
        out = torch.empty(B, Tmax, Nmax, device=self.device, dtype=torch.float32)
        check(lib.radmmm_prior_zoom_batch(ptr(items), B, ptr(out), Tmax, Nmax, stream()), "prior_zoom_batch")
        return out

    def __call__(self, p_count: int, m_count: int) -> torch.Tensor:
        """[m_count, p_count] fp32 prior of one utterance."""
        return self.batch([p_count], [m_count])[0]


def get_energy_average(mel: torch.Tensor, use_scaled_energy: bool = True) -> torch.Tensor:
    """data.py:363-366 (+ energy_avg_normalize :339-342): mel [n_mel, T] or [B, n_mel, T] fp32 -> [T] / [B, T]."""
    single = mel.dim() == 2
    m = (mel[None] if single else mel).float().contiguous()
    B, n_mel, T = m.shape
    out = torch.empty(B, T, device=m.device, dtype=torch.float32)
    check(lib.radmmm_energy_average(ptr(m), ptr(out), B, n_mel, T, 1 if use_scaled_energy else 0, stream()), "energy_average")
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------------
# Whole training batches on the device (data.py:419-610 __getitem__ after the file reads, :616-790 DataCollate):
# csrc/collate.hip, DESIGN.md 4.18
# ---------------------------------------------------------------------------------------------------------------------
_TRACKS = ("f0", "p_voiced", "voiced_mask")
_SPEAKER_STATS = ("speaker_f0_mean", "speaker_f0_std", "speaker_energy_mean", "speaker_energy_std")
_SAMPLE_ALIGN = 8          # samples between item starts in the staging buffer are padded to this (16 bytes of int16)


def _host_array(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise ValueError("items hold host data (numpy arrays or CPU tensors); the batch is built on the device from them")
        x = x.detach().numpy()
    return np.asarray(x)


def _r(n: int, to: int) -> int:
    return (n + to - 1) // to * to


@dataclass
class BatchPlan:
    """Where every item of a batch goes (plan_batch).  All per-item arrays are in SORTED order; `order[i]` is the index
    into the caller's list of the item in row i."""
    order: List[int]
    input_lengths: np.ndarray           # int64 [B] token counts
    output_lengths: np.ndarray          # int64 [B] frame counts, 1 + S // hop
    audio_lengths: np.ndarray           # int64 [B] sample counts
    sample_offsets: np.ndarray          # int64 [B] first sample of the item in the packed sample section
    frame_offsets: np.ndarray           # int64 [B] first frame in each packed track
    token_offsets: np.ndarray           # int64 [B] first id in the packed ids
    Smax: int
    Tmax: int
    Lmax: int
    n_samples: int                      # lengths of the packed sections (elements)
    n_frames: int
    n_tokens: int
    audio_dtype: np.dtype               # int16 or float32: one per batch
    tracks: Tuple[str, ...]             # which of f0 / p_voiced / voiced_mask the items carry


def plan_batch(items: Sequence[dict], hop_length: int, filter_length: int = 1024) -> BatchPlan:
    """Host-side layout of a batch (no GPU needed).  items: dicts as the reference's __getitem__ has them BEFORE its feature
    computation: audio (1-D int16 or float32 samples at the wav file's scale), text_encoded (1-D ids), optional raw f0 /
    p_voiced / voiced_mask as cached from pyin (1-D, one value per frame), speaker_id, accent_id, optional speaker_* stats
    and the pass-through idx / audiopath / text_raw / language.  Rows are ordered by torch.sort(text lengths,
    descending=True), the call DataCollate makes (data.py:629-631), so ties fall the same way."""
    if len(items) == 0:
        raise ValueError("plan_batch: empty batch")
    hop_length, filter_length = int(hop_length), int(filter_length)
    n_tok = [int(_host_array(it["text_encoded"]).shape[0]) for it in items]
    input_lengths, order = torch.sort(torch.LongTensor(n_tok), dim=0, descending=True)
    order = [int(v) for v in order]
    tracks = tuple(k for k in _TRACKS if items[order[0]].get(k) is not None)
    dtypes, S, T = set(), [], []
    for i in order:
        it = items[i]
        a = _host_array(it["audio"])
        if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
            raise ValueError(f"plan_batch: item {i}: audio must be 1-D int16 or float32 samples (got {a.dtype}, {a.ndim}-D)")
        dtypes.add(a.dtype)
        s = int(a.shape[0])
        if s <= filter_length // 2:
            raise ValueError(f"plan_batch: item {i}: {s} samples; the reflect pad of the STFT needs more than "
                             f"filter_length // 2 = {filter_length // 2}")
        if n_tok[i] < 1:
            raise ValueError(f"plan_batch: item {i}: empty text")
        t = 1 + s // hop_length
        for k in _TRACKS:
            v = it.get(k)
            if (v is not None) != (k in tracks):
                raise ValueError(f"plan_batch: item {i}: {k} must be given for every item of the batch or for none")
            if v is not None and tuple(_host_array(v).shape) != (t,):
                raise ValueError(f"plan_batch: item {i}: {k} has shape {tuple(_host_array(v).shape)}, the utterance has "
                                 f"{t} frames (1 + {s} // {hop_length})")
        S.append(s)
        T.append(t)
    if len(dtypes) != 1:
        raise ValueError("plan_batch: int16 and float32 audio mixed in one batch")
    L = [int(v) for v in input_lengths]
    so, fo, to = [0], [0], [0]
    for s, t, l in zip(S, T, L):
        so.append(so[-1] + _r(s, _SAMPLE_ALIGN))
        fo.append(fo[-1] + t)
        to.append(to[-1] + l)
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    return BatchPlan(order=order, input_lengths=i64(L), output_lengths=i64(T), audio_lengths=i64(S),
                     sample_offsets=i64(so[:-1]), frame_offsets=i64(fo[:-1]), token_offsets=i64(to[:-1]),
                     Smax=max(S), Tmax=max(T), Lmax=max(L), n_samples=so[-1], n_frames=fo[-1], n_tokens=to[-1],
                     audio_dtype=dtypes.pop(), tracks=tracks)


class _Grow:
    """A buffer that is kept between calls and only ever grows."""

    def __init__(self):
        self.t: Optional[torch.Tensor] = None

    def get(self, n: int, **kw) -> torch.Tensor:
        if self.t is None or self.t.numel() < n:
            self.t = torch.empty(n + n // 8, **kw)
        return self.t


def _tracks_call(f0p, pvp, vmp, ids, frame_off, tok_off, frames, in_lens, f0, pv, vm, text, scan, meta_src, meta_dst,
                 n_meta, B, Tmax, Lmax, f0_min, use_log_f0, distance_tx):
    check(lib.radmmm_collate_tracks(ptr(f0p), ptr(pvp), ptr(vmp), ptr(ids), ptr(frame_off), ptr(tok_off), ptr(frames),
                                    ptr(in_lens), ptr(f0), ptr(pv), ptr(vm), ptr(text), ptr(scan), ptr(meta_src),
                                    ptr(meta_dst), int(n_meta), int(B), int(Tmax), int(Lmax), float(f0_min),
                                    1 if use_log_f0 else 0, 1 if distance_tx else 0, stream()), "collate_tracks")


def _padded_rows(f0: torch.Tensor):
    if not f0.is_cuda:
        raise RadmmmError("rad_mmm_amd.data needs GPU tensors (there is no CPU path)")
    if f0.dim() != 2:
        raise ValueError("expected a padded [B, T] tensor")
    x = f0.float().contiguous()
    B, T = x.shape
    off = torch.arange(B, device=x.device, dtype=torch.int64) * T
    return x, B, T, off


def f0_normalize(f0: torch.Tensor, f0_min: float, use_log_f0: bool = True) -> torch.Tensor:
    """data.py:321-327 on a padded device tensor [B, T] (Hz, 0 where unvoiced): log(x) where x >= f0_min, else 0; the
    input itself with use_log_f0 off.  Returns a new tensor."""
    x, B, T, off = _padded_rows(f0)
    out = torch.empty_like(x)
    frames = torch.full((B,), T, device=x.device, dtype=torch.int32)
    _tracks_call(x, None, None, None, off, None, frames, None, out, None, None, None, None, None, None, 0, B, T, 0,
                 f0_min, use_log_f0, False)
    return out


def f0_denormalize(f0: torch.Tensor, f0_min: float, use_log_f0: bool = True) -> torch.Tensor:
    """data.py:329-337: exp(x) where x >= log(f0_min) (log f0), everything <= 0 set to 0.  Returns a new tensor."""
    if not f0.is_cuda:
        raise RadmmmError("rad_mmm_amd.data needs GPU tensors (there is no CPU path)")
    x = f0.float()
    if use_log_f0:
        x = torch.where(x >= float(np.log(f0_min)), torch.exp(x), torch.zeros_like(x))
    return torch.clamp_min(x, 0.0)


def distance_tx_unvoiced(f0: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """data.py:527-532 on a padded batch: f0 [B, T] already normalised (f0 <= 0 where unvoiced), lens [B] frame counts on
    the device.  f0 - max(log(d), 0), d the distance in frames to the nearest voiced frame of the same utterance; zeros
    past each length.  An utterance without a voiced frame gets d = t + 1 (what scipy returns)."""
    x, B, T, off = _padded_rows(f0)
    if not lens.is_cuda or lens.numel() != B:
        raise ValueError("lens: a device tensor of B frame counts")
    out = torch.empty_like(x)
    scan = torch.empty(B, T, device=x.device, dtype=torch.int32)
    _tracks_call(x, None, None, None, off, None, lens.to(torch.int32), None, out, None, None, None, scan, None, None, 0,
                 B, T, 0, 0.0, False, True)
    return out


class DeviceCollate:
    """AudioDataset.__getitem__'s feature computation and DataCollate in one place, on the device: raw items in (see
    plan_batch), the batch dictionary of data.py:756-788 out -- mel, text, input_lengths, output_lengths, speaker_ids,
    accent_ids, attn_prior, energy_avg, f0, p_voiced, voiced_mask, the four speaker_* vectors, idx, the pass-through lists,
    plus input_lengths_host / output_lengths_host (TTSTrainingStep reads them instead of the device copies) and, with
    return_audio, audio [B, 1, Smax] and audio_lengths.  Rows are sorted by text length (descending), zeros past every
    length.  One pinned staging buffer and one host -> device copy per call, no device -> host read; kernels run on the
    current stream.  Staging and scratch buffers are kept between calls (two staging buffers in rotation: the host may
    fill the next batch while the previous copy is in flight); the returned tensors are fresh.

    `stft` is a rad_mmm_amd.audio_processing.TacotronSTFT on the device.  Use as the collate function of a DataLoader in
    the main process (`collate_fn=lambda x: x` in the workers)."""

    def __init__(self, stft, max_wav_value: float = 32768.0, f0_min: float = 80.0, use_log_f0: bool = True,
                 distance_tx_unvoiced: bool = False, use_scaled_energy: bool = True, use_attn_prior_masking: bool = True,
                 prior: Optional[BetaBinomialInterpolator] = None, return_audio: bool = False):
        dev = stft.mel_basis.device
        if dev.type != "cuda":
            raise RuntimeError("DeviceCollate: move the TacotronSTFT to the GPU first (there is no CPU path)")
        self.stft = stft
        self.device = dev
        self.max_wav_value = float(max_wav_value)
        self.f0_min = float(f0_min)
        self.use_log_f0 = bool(use_log_f0)
        self.distance_tx_unvoiced = bool(distance_tx_unvoiced)
        self.use_scaled_energy = bool(use_scaled_energy)
        self.use_attn_prior_masking = bool(use_attn_prior_masking)
        self.prior = prior if prior is not None else (BetaBinomialInterpolator(device=dev) if use_attn_prior_masking else None)
        self.return_audio = bool(return_audio)
        self._slots = [{"host": _Grow(), "event": None}, {"host": _Grow(), "event": None}]
        self._turn = 0
        self._dev_staging, self._scratch, self._scan = _Grow(), _Grow(), _Grow()
        self._last_stream = None
        # measurement hook (tools/collate_bench.py): a list collects one (start, end) pair of timing events per call around
        # the device work alone -- the copy and the kernels, not the host's filling of the staging buffer
        self.timing_events: Optional[list] = None

    # ---- staging layout: 16-byte aligned sections of one byte buffer ---------------------------------------------------
    @staticmethod
    def _layout(plan: BatchPlan):
        B = len(plan.order)
        n_meta = 6 * B + (4 * B + 1) // 2                  # int64 rows, then 4 fp32 rows, in 8-byte words
        sizes = [("offsets", 3 * B * 8), ("lens", 3 * B * 4), ("meta", n_meta * 8), ("ids", plan.n_tokens * 4)]
        sizes += [(k, plan.n_frames * 4) for k in plan.tracks]
        sizes.append(("audio", plan.n_samples * plan.audio_dtype.itemsize))
        off, o = {}, 0
        for k, n in sizes:
            off[k] = (o, n)
            o += _r(n, 16)
        return off, o, n_meta

    def __call__(self, items: Sequence[Optional[dict]]) -> Optional[dict]:
        items = [it for it in items if it is not None]
        if len(items) == 0:
            return None
        s = self.stft.stft_fn
        plan = plan_batch(items, s.hop_length, s.filter_length)
        B, dev = len(items), self.device
        off, total, n_meta = self._layout(plan)

        cur = torch.cuda.current_stream(dev)
        if self._last_stream is not None and self._last_stream != cur:
            cur.wait_stream(self._last_stream)               # the kept buffers were last used there
        self._last_stream = cur

        slot = self._slots[self._turn]
        self._turn ^= 1
        if slot["event"] is not None:
            slot["event"].synchronize()                      # its previous host -> device copy (two calls ago) has left
        host = slot["host"].get(total, dtype=torch.uint8, pin_memory=True)
        hb = host.numpy()

        def sec(name, dtype):
            o, n = off[name]
            return hb[o:o + n].view(dtype)
        offs = sec("offsets", np.int64).reshape(3, B)
        offs[0], offs[1], offs[2] = plan.sample_offsets, plan.frame_offsets, plan.token_offsets
        lens = sec("lens", np.int32).reshape(3, B)
        lens[0], lens[1], lens[2] = plan.audio_lengths, plan.output_lengths, plan.input_lengths
        meta = sec("meta", np.int64)
        mi = meta[:6 * B].reshape(6, B)
        mf = meta[6 * B:].view(np.float32)[:4 * B].reshape(4, B)
        mi[0], mi[1], mi[5] = plan.input_lengths, plan.output_lengths, plan.audio_lengths
        ids = sec("ids", np.int32)
        trk = {k: sec(k, np.float32) for k in plan.tracks}
        audio = sec("audio", plan.audio_dtype)
        for r, i in enumerate(plan.order):
            it = items[i]
            mi[2, r], mi[3, r], mi[4, r] = int(it["speaker_id"]), int(it["accent_id"]), int(it.get("idx", 0))
            for c, k in enumerate(_SPEAKER_STATS):
                v = it.get(k)
                mf[c, r] = 0.0 if v is None else float(v)
            t = _host_array(it["text_encoded"])
            if t.size and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
                raise ValueError(f"DeviceCollate: item {i}: token ids do not fit 32 bits")
            ids[plan.token_offsets[r]:plan.token_offsets[r] + t.shape[0]] = t
            fo, nt = plan.frame_offsets[r], plan.output_lengths[r]
            for k in plan.tracks:
                trk[k][fo:fo + nt] = _host_array(it[k])
            so, ns = plan.sample_offsets[r], plan.audio_lengths[r]
            audio[so:so + ns] = _host_array(it["audio"])

        dbuf = self._dev_staging.get(total, dtype=torch.uint8, device=dev)
        if self.timing_events is not None:
            self.timing_events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            self.timing_events[-1][0].record(cur)
        dbuf[:total].copy_(host[:total], non_blocking=True)
        if slot["event"] is None:
            slot["event"] = torch.cuda.Event()
        slot["event"].record(cur)

        def dsec(name, dtype):
            o, n = off[name]
            return dbuf[o:o + n].view(dtype)
        d_offs = dsec("offsets", torch.int64).view(3, B)
        d_lens = dsec("lens", torch.int32).view(3, B)
        n_mel, Tmax, Lmax, Smax = self.stft.n_mel_channels, plan.Tmax, plan.Lmax, plan.Smax

        f32 = dict(device=dev, dtype=torch.float32)
        mel = torch.empty(B, n_mel, Tmax, **f32)
        energy = torch.empty(B, Tmax, **f32)
        audio_out = torch.empty(B, 1, Smax, **f32) if self.return_audio else None
        scratch = self._scratch.get(int(lib.radmmm_collate_scratch_floats(B, Smax, s.filter_length, s.hop_length, n_mel)), **f32)
        o, n = off["audio"]
        packed = dbuf[o:o + n].view(torch.int16 if plan.audio_dtype == np.int16 else torch.float32)
        self.stft.mel_spectrogram_ragged(packed, plan.audio_lengths, mel, lens_device=d_lens[0], frames_device=d_lens[1],
                                         offsets=d_offs[0], scale=1.0 / self.max_wav_value, energy=energy,
                                         scaled_energy=self.use_scaled_energy, audio_out=audio_out, scratch=scratch)

        text = torch.empty(B, Lmax, device=dev, dtype=torch.int64)
        meta_out = torch.empty(n_meta, device=dev, dtype=torch.int64)
        out_trk = {k: torch.empty(B, Tmax, **f32) for k in plan.tracks}
        d_trk = {k: dsec(k, torch.float32) for k in plan.tracks}
        need_scan = "f0" in plan.tracks and self.distance_tx_unvoiced
        scan = self._scan.get(B * Tmax, device=dev, dtype=torch.int32) if need_scan else None
        _tracks_call(d_trk.get("f0"), d_trk.get("p_voiced"), d_trk.get("voiced_mask"), dsec("ids", torch.int32), d_offs[1],
                     d_offs[2], d_lens[1], d_lens[2], out_trk.get("f0"), out_trk.get("p_voiced"), out_trk.get("voiced_mask"),
                     text, scan, dsec("meta", torch.int64), meta_out, n_meta, B, Tmax, Lmax, self.f0_min, self.use_log_f0,
                     self.distance_tx_unvoiced)

        oi = meta_out[:6 * B].view(6, B)
        of = meta_out[6 * B:].view(torch.float32)[:4 * B].view(4, B)
        in_host, out_host = torch.from_numpy(plan.input_lengths.copy()), torch.from_numpy(plan.output_lengths.copy())
        attn_prior = self.prior.batch(in_host.tolist(), out_host.tolist()) if self.use_attn_prior_masking else None
        batch = {"mel": mel, "speaker_ids": oi[2], "accent_ids": oi[3],
                 "text_raw": [items[i].get("text_raw") for i in plan.order],
                 "language": [items[i].get("language") for i in plan.order],
                 "text": text, "input_lengths": oi[0], "output_lengths": oi[1],
                 "audiopaths": [items[i].get("audiopath") for i in plan.order],
                 "attn_prior": attn_prior, "idx": oi[4],
                 "speaker_f0_mean": of[0], "speaker_f0_std": of[1], "speaker_energy_mean": of[2],
                 "speaker_energy_std": of[3],
                 "input_lengths_host": in_host, "output_lengths_host": out_host,
                 "energy_avg": energy}
        if self.return_audio:
            batch["audio"] = audio_out
            batch["audio_lengths"] = oi[5]
        batch.update(out_trk)
        if self.timing_events is not None:
            self.timing_events[-1][1].record(cur)
        return batch


# ---------------------------------------------------------------------------------------------------------------------
# Random fixed-length segments for vocoder training (upstream HiFi-GAN's meldataset: segment_size 8192): the crop happens
# on the host while the staging buffer is filled, the unpack and the mel are DeviceCollate's kernels
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class SegmentPlan:
    """Where every item's segment comes from and goes (plan_segments); rows in the caller's order."""
    starts: np.ndarray                  # int64 [B] first sample of the crop inside the item
    counts: np.ndarray                  # int64 [B] samples staged, min(S_b - start, segment_size)
    lens: np.ndarray                    # int64 [B] mel frames, counts // hop
    offsets: np.ndarray                 # int64 [B] first sample of the crop in the packed sample section
    n_samples: int                      # length of the packed section (elements)
    segment_size: int
    audio_dtype: np.dtype               # int16 or float32: one per batch


def plan_segments(items: Sequence[dict], hop_length: int, filter_length: int = 1024, segment_size: int = 8192,
                  starts: Optional[Sequence[int]] = None, generator: Optional[torch.Generator] = None) -> SegmentPlan:
    """Host-side layout of a batch of segments (no GPU needed).  items: dicts with `audio`, 1-D int16 or float32 host
    samples as plan_batch takes them.  starts: one per item, or None: drawn from `generator` (a CPU torch.Generator, None:
    torch's default), uniformly from 0 .. S_b - segment_size (0 for an item shorter than the segment, which is staged whole).
    Every staged range must hold more than filter_length // 2 samples, the reflect pad of the STFT."""
    hop_length, filter_length, segment_size = int(hop_length), int(filter_length), int(segment_size)
    if len(items) == 0:
        raise ValueError("plan_segments: empty batch")
    if segment_size <= filter_length // 2 or segment_size % hop_length:
        raise ValueError(f"plan_segments: segment_size {segment_size} must be a multiple of hop_length {hop_length} above "
                         f"filter_length // 2 = {filter_length // 2}")
    if starts is not None and len(starts) != len(items):
        raise ValueError(f"plan_segments: {len(starts)} starts for {len(items)} items")
    dtypes, st, cnt = set(), [], []
    for i, it in enumerate(items):
        a = _host_array(it["audio"])
        if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
            raise ValueError(f"plan_segments: item {i}: audio must be 1-D int16 or float32 samples (got {a.dtype}, {a.ndim}-D)")
        dtypes.add(a.dtype)
        s = int(a.shape[0])
        if s <= filter_length // 2:
            raise ValueError(f"plan_segments: item {i}: {s} samples; the reflect pad of the STFT needs more than "
                             f"filter_length // 2 = {filter_length // 2}")
        if starts is not None:
            b = int(starts[i])
            if not 0 <= b < s:
                raise ValueError(f"plan_segments: item {i}: start {b} outside its {s} samples")
        else:
            hi = max(s - segment_size, 0)
            b = int(torch.randint(0, hi + 1, (1,), generator=generator)) if hi > 0 else 0
        n = min(s - b, segment_size)
        if n <= filter_length // 2:
            raise ValueError(f"plan_segments: item {i}: start {b} leaves {n} samples; the reflect pad of the STFT needs more "
                             f"than filter_length // 2 = {filter_length // 2}")
        st.append(b)
        cnt.append(n)
    if len(dtypes) != 1:
        raise ValueError("plan_segments: int16 and float32 audio mixed in one batch")
    so = [0]
    for n in cnt:
        so.append(so[-1] + _r(n, _SAMPLE_ALIGN))
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    return SegmentPlan(starts=i64(st), counts=i64(cnt), lens=i64(cnt) // hop_length, offsets=i64(so[:-1]), n_samples=so[-1],
                       segment_size=segment_size, audio_dtype=dtypes.pop())


def segment_layout(plan: SegmentPlan):
    """({section: (byte offset, bytes)}, total bytes) of the staging buffer: 16-byte aligned sections"""
    B = len(plan.starts)
    off, o = {}, 0
    for k, n in (("offsets", B * 8), ("lens", 2 * B * 4), ("audio", plan.n_samples * plan.audio_dtype.itemsize)):
        off[k] = (o, n)
        o += _r(n, 16)
    return off, o


def stage_segments(plan: SegmentPlan, items: Sequence[dict], hb: np.ndarray) -> int:
    """Fill the staging bytes `hb` (uint8, at least segment_layout(plan)[1] long): the packed offsets, the sample and frame
    counts, and the cropped samples alone -- item b's [start, start + count).  Returns the bytes used."""
    off, total = segment_layout(plan)
    B = len(plan.starts)

    def sec(name, dtype):
        o, n = off[name]
        return hb[o:o + n].view(dtype)
    sec("offsets", np.int64)[:] = plan.offsets
    lens = sec("lens", np.int32).reshape(2, B)
    lens[0], lens[1] = plan.counts, plan.lens
    audio = sec("audio", plan.audio_dtype)
    for b, it in enumerate(items):
        s, n, o = int(plan.starts[b]), int(plan.counts[b]), int(plan.offsets[b])
        audio[o:o + n] = _host_array(it["audio"])[s:s + n]
    return total


class SegmentCollate:
    """Batches of fixed-length segments for vocoder training, on the device: SegmentCollate(stft, segment_size, generator)
    (items, starts=None) -> {"mel" [B, n_mel, segment_size // hop], "audio" [B, 1, segment_size], "lens" [B] valid frames
    (int32, device), "lens_host" (int64 CPU tensor)}, rows in the caller's order.  Item b contributes its samples
    [start, start + segment_size) (plan_segments); a shorter item is staged whole and zero-padded on the right, lens[b] =
    min(S_b - start, segment_size) // hop.  The mel is the first segment_size // hop frames of the ragged log-mel of the
    segments at their valid sample counts (stft.mel_spectrogram_ragged, each item reflect-padded at its own two ends), exact
    zeros from frame lens[b] on.  int16 samples are scaled by 1 / max_wav_value.

    Only the cropped ranges go through the pinned staging buffer: one host -> device copy per call, no device -> host read;
    the unpack and the mel are DeviceCollate's kernels, and the buffers are kept between calls in the same way."""

    def __init__(self, stft, segment_size: int = 8192, generator: Optional[torch.Generator] = None,
                 max_wav_value: float = 32768.0):
        dev = stft.mel_basis.device
        if dev.type != "cuda":
            raise RuntimeError("SegmentCollate: move the TacotronSTFT to the GPU first (there is no CPU path)")
        s = stft.stft_fn
        if int(segment_size) <= s.filter_length // 2 or int(segment_size) % s.hop_length:
            raise ValueError(f"SegmentCollate: segment_size {segment_size} must be a multiple of hop_length {s.hop_length} "
                             f"above filter_length // 2 = {s.filter_length // 2}")
        self.stft, self.device, self.segment_size, self.generator = stft, dev, int(segment_size), generator
        self.max_wav_value = float(max_wav_value)
        self._slots = [{"host": _Grow(), "event": None}, {"host": _Grow(), "event": None}]
        self._turn = 0
        self._dev_staging, self._scratch = _Grow(), _Grow()
        self._last_stream = None

    def __call__(self, items: Sequence[dict], starts: Optional[Sequence[int]] = None) -> dict:
        s = self.stft.stft_fn
        hop, n_mel, seg, dev = s.hop_length, self.stft.n_mel_channels, self.segment_size, self.device
        plan = plan_segments(items, hop, s.filter_length, seg, starts, self.generator)
        B = len(items)
        off, total = segment_layout(plan)

        cur = torch.cuda.current_stream(dev)
        if self._last_stream is not None and self._last_stream != cur:
            cur.wait_stream(self._last_stream)               # the kept buffers were last used there
        self._last_stream = cur
        slot = self._slots[self._turn]
        self._turn ^= 1
        if slot["event"] is not None:
            slot["event"].synchronize()                      # its previous host -> device copy (two calls ago) has left
        host = slot["host"].get(total, dtype=torch.uint8, pin_memory=True)
        stage_segments(plan, items, host.numpy())
        dbuf = self._dev_staging.get(total, dtype=torch.uint8, device=dev)
        dbuf[:total].copy_(host[:total], non_blocking=True)
        if slot["event"] is None:
            slot["event"] = torch.cuda.Event()
        slot["event"].record(cur)

        def dsec(name, dtype):
            o, n = off[name]
            return dbuf[o:o + n].view(dtype)
        d_lens = dsec("lens", torch.int32).view(2, B)
        packed = dsec("audio", torch.int16 if plan.audio_dtype == np.int16 else torch.float32)
        Smax = int(plan.counts.max())
        F = seg // hop
        f32 = dict(device=dev, dtype=torch.float32)
        audio = torch.empty(B, 1, Smax, **f32)
        scratch = self._scratch.get(int(lib.radmmm_collate_scratch_floats(B, Smax, s.filter_length, hop, n_mel)), **f32)
        # frames_device = lens: the ragged mel's last frame of an item, 1 + count // hop, is cut (exact zeros from lens[b] on)
        mel = self.stft.mel_spectrogram_ragged(packed, plan.counts, None, lens_device=d_lens[0], frames_device=d_lens[1],
                                               offsets=dsec("offsets", torch.int64), scale=1.0 / self.max_wav_value
                                               if plan.audio_dtype == np.int16 else 1.0, audio_out=audio, scratch=scratch)
        if Smax == seg:
            mel = mel[:, :, :F].contiguous()
        else:                                                # every item is shorter than the segment
            mel = torch.nn.functional.pad(mel[:, :, :F], (0, F - min(F, mel.shape[2])))
            audio = torch.nn.functional.pad(audio, (0, seg - Smax))
        return {"mel": mel, "audio": audio, "lens": d_lens[1].clone(), "lens_host": torch.from_numpy(plan.lens.copy())}
