// Training batches built on the device (reference data.py:419-610 AudioDataset.__getitem__, :616-790 DataCollate):
// one packed staging buffer of ragged utterances in, the padded tensors of the batch dictionary out.
//   unpack_pad   packed int16 / fp32 samples -> reflect-padded, scaled fp32 rows (the STFT GEMM's A operand), and the
//                padded `audio` of the batch in the same pass
//   finish       melT rows -> log-mel [B, n_mel, Tmax] with zeros past each length, and the energy average beside it
//   tracks       f0 transform (log above f0_min, minus log of the distance to the nearest voiced frame), p_voiced,
//                voiced_mask, token ids and the small per-item scalars
// The two GEMMs between unpack_pad and finish are the radmmm_rowgemm_f32 launches of radmmm_stft_mel (stft_kernels.h).
#include <limits.h>

#include "common.h"
#include "stft_kernels.h"

namespace {

__device__ __forceinline__ float sample_at(const void* __restrict__ src, int is_i16, long long i, float scale) {
  return is_i16 ? (float)static_cast<const short*>(src)[i] * scale : static_cast<const float*>(src)[i] * scale;
}

// xpad[b][p] = src[off[b] + reflect(p - pad)] * scale for p < lens[b] + 2 pad, 0 beyond; four samples per lane (one
// 16-byte store).  Lanes whose four samples lie inside the utterance at a 4-sample-aligned source position (all but the
// two reflected ends, when the item offsets are multiples of 4) take them with one 8- or 16-byte load.
// audio != nullptr: audio[b][j] = src[off[b] + j] * scale for j < lens[b], 0 up to Smax (row pitch Smax).
__global__ __launch_bounds__(256) void unpack_pad_kernel(const void* __restrict__ src, int is_i16,
                                                         const long long* __restrict__ off,
                                                         const int* __restrict__ lens, float* __restrict__ xpad,
                                                         float* __restrict__ audio, int pad, int pitch, int Smax,
                                                         float scale) {
  const int b = blockIdx.y;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= pitch) return;
  const int S = lens[b];
  const long long o = off[b];
  const int j0 = p0 - pad;
  float v[4];
  if (j0 >= 0 && j0 + 3 < S && ((o + j0) & 3) == 0) {
    if (is_i16) {
      const short4 q = *reinterpret_cast<const short4*>(static_cast<const short*>(src) + o + j0);
      v[0] = (float)q.x * scale; v[1] = (float)q.y * scale; v[2] = (float)q.z * scale; v[3] = (float)q.w * scale;
    } else {
      const float4 q = *reinterpret_cast<const float4*>(static_cast<const float*>(src) + o + j0);
      v[0] = q.x * scale; v[1] = q.y * scale; v[2] = q.z * scale; v[3] = q.w * scale;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = p0 + k;
      float x = 0.f;
      if (p < S + 2 * pad) {
        int j = p - pad;
        if (j < 0) j = -j;                    // reflect (no edge repeat); S > pad keeps both inside [0, S)
        if (j >= S) j = 2 * (S - 1) - j;
        j = min(max(j, 0), S - 1);            // (a caller that breaks S > pad reads a wrong sample, never out of bounds)
        x = sample_at(src, is_i16, o + j, scale);
      }
      v[k] = x;
    }
  }
  *reinterpret_cast<float4*>(xpad + (long long)b * pitch + p0) = make_float4(v[0], v[1], v[2], v[3]);
  if (audio) {
    float* ap = audio + (long long)b * Smax;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k;
      if (j >= 0 && j < Smax) ap[j] = j < S ? v[k] : 0.f;      // (j < S here is never a reflected sample: p = j + pad)
    }
  }
}

// One lane per frame: mel[b][c][t] = log(max(melT[(b*Tmax + t)*ldt + c], clip)) for t < frames[b], else 0; the energy
// average sums the channels in ascending order in fp32, divides by n_mel, then (x + 20) / 20 when scaled -- operation
// for operation what energy_average_kernel (prior.hip) does on the finished mel, so the two agree bit for bit.
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ melT, int ldt,
                                                     const int* __restrict__ frames, float* __restrict__ mel,
                                                     float* __restrict__ energy, int Tmax, int n_mel, float clip,
                                                     int scaled) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Tmax) return;
  float* mp = mel + (long long)b * n_mel * Tmax + t;
  if (t >= frames[b]) {
    for (int c = 0; c < n_mel; ++c) mp[(long long)c * Tmax] = 0.f;
    if (energy) energy[(long long)b * Tmax + t] = 0.f;
    return;
  }
  const float* row = melT + ((long long)b * Tmax + t) * ldt;
  float s = 0.f;
  int c = 0;
  for (; c + 3 < n_mel; c += 4) {                              // ldt % 4 == 0 and a 16-byte aligned base: float4 rows
    const float4 q = *reinterpret_cast<const float4*>(row + c);
    const float l0 = logf(fmaxf(q.x, clip)), l1 = logf(fmaxf(q.y, clip)), l2 = logf(fmaxf(q.z, clip)),
                l3 = logf(fmaxf(q.w, clip));
    mp[(long long)c * Tmax] = l0;
    mp[(long long)(c + 1) * Tmax] = l1;
    mp[(long long)(c + 2) * Tmax] = l2;
    mp[(long long)(c + 3) * Tmax] = l3;
    s += l0; s += l1; s += l2; s += l3;
  }
  for (; c < n_mel; ++c) {
    const float l = logf(fmaxf(row[c], clip));
    mp[(long long)c * Tmax] = l;
    s += l;
  }
  if (energy) {
    float e = s / (float)n_mel;
    if (scaled) e = (e + 20.0f) / 20.0f;
    energy[(long long)b * Tmax + t] = e;
  }
}

// inclusive scans over the 256 lanes of a workgroup (4 waves): wave scan by shuffles, the wave totals through LDS
__device__ __forceinline__ int block_scan_max_fwd(int v, int* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v = max(v, u);
  }
  __syncthreads();
  if (lane == 63) sh[w] = v;
  __syncthreads();
  for (int k = 0; k < w; ++k) v = max(v, sh[k]);
  return v;
}
__device__ __forceinline__ int block_scan_min_bwd(int v, int* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_down(v, o, 64);
    if (lane + o < 64) v = min(v, u);
  }
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  for (int k = w + 1; k < 4; ++k) v = min(v, sh[k]);
  return v;
}

__device__ __forceinline__ float f0_norm(float x, float f0_min, int use_log) {
  // data.py:321-327; the log is taken in double and rounded once (correctly rounded fp32 log)
  if (!use_log) return x;
  return x >= f0_min ? (float)log((double)x) : 0.f;
}

// One workgroup per utterance.  The distance to the nearest voiced frame (f0 > 0 after f0_norm) is
// min(t - last voiced index at or before t, next voiced index at or after t - t): a forward max-scan and a backward
// min-scan over chunks of 256 frames with a carry between chunks, so any T works.  The forward pass parks the normalised
// f0 in the output row and `last` in `scan`; each lane reads back only what it wrote itself.
__global__ __launch_bounds__(256) void tracks_kernel(const float* __restrict__ f0p, const float* __restrict__ pvp,
                                                     const float* __restrict__ vmp, const int* __restrict__ ids,
                                                     const long long* __restrict__ frame_off,
                                                     const long long* __restrict__ tok_off,
                                                     const int* __restrict__ frames, const int* __restrict__ in_lens,
                                                     float* __restrict__ f0, float* __restrict__ pv,
                                                     float* __restrict__ vm, long long* __restrict__ text,
                                                     int* __restrict__ scan, const long long* __restrict__ meta_src,
                                                     long long* __restrict__ meta_dst, int n_meta, int Tmax, int Lmax,
                                                     float f0_min, int use_log, int dist_tx) {
  __shared__ int sh[4];
  __shared__ int sh_carry;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = frames[b];
  const long long fo = frame_off[b];
  for (int i = b * 256 + tid; i < n_meta; i += gridDim.x * 256) meta_dst[i] = meta_src[i];
  if (text) {
    const int L = in_lens[b];
    const long long to = tok_off[b];
    for (int l = tid; l < Lmax; l += 256) text[(long long)b * Lmax + l] = l < L ? (long long)ids[to + l] : 0LL;
  }
  for (int t = tid; t < Tmax; t += 256) {
    const bool in = t < T;
    if (pv) pv[(long long)b * Tmax + t] = in ? pvp[fo + t] : 0.f;
    if (vm) vm[(long long)b * Tmax + t] = in ? vmp[fo + t] : 0.f;
  }
  if (!f0) return;
  float* fr = f0 + (long long)b * Tmax;
  if (!dist_tx) {
    for (int t = tid; t < Tmax; t += 256) fr[t] = t < T ? f0_norm(f0p[fo + t], f0_min, use_log) : 0.f;
    return;
  }
  int* sr = scan + (long long)b * Tmax;
  const int nchunk = (T + 255) / 256;
  int carry = -1;
  for (int c = 0; c < nchunk; ++c) {
    const int t = c * 256 + tid;
    float x = 0.f;
    if (t < T) x = f0_norm(f0p[fo + t], f0_min, use_log);
    int last = block_scan_max_fwd((t < T && x > 0.f) ? t : -1, sh);
    last = max(last, carry);
    if (t < T) {
      fr[t] = x;
      sr[t] = last;
    }
    if (tid == 255) sh_carry = last;
    __syncthreads();
    carry = sh_carry;
  }
  const bool none_voiced = carry < 0;               // scipy's transform without any background: d = t + 1
  carry = INT_MAX;
  for (int c = nchunk - 1; c >= 0; --c) {
    const int t = c * 256 + tid;
    float x = 0.f;
    int last = -1;
    if (t < T) {
      x = fr[t];
      last = sr[t];
    }
    int next = block_scan_min_bwd((t < T && x > 0.f) ? t : INT_MAX, sh);
    next = min(next, carry);
    if (t < T) {
      int d;
      if (none_voiced) {
        d = t + 1;
      } else {
        d = INT_MAX;
        if (last >= 0) d = t - last;
        if (next != INT_MAX) d = min(d, next - t);
      }
      // data.py:527-532: float32 f0 minus a float64 map, rounded when DataCollate copies it into a FloatTensor
      const double dm = d > 1 ? log((double)d) : 0.0;
      fr[t] = (float)((double)x - dm);
    }
    __syncthreads();                                 // every lane has read sh_carry of the previous round
    if (tid == 0) sh_carry = next;
    __syncthreads();
    carry = sh_carry;
  }
  for (int t = T + tid; t < Tmax; t += 256) fr[t] = 0.f;
}

}  // namespace

extern "C" int64_t radmmm_collate_scratch_floats(int B, int Smax, int n_fft, int hop, int n_mel) {
  return stft_layout(B, Smax, n_fft, hop, n_mel).total;
}

extern "C" int radmmm_collate_unpack_pad(const void* src, int src_int16, const int64_t* offsets, const int32_t* lens,
                                         float* scratch, float* audio, int B, int Smax, int n_fft, float scale,
                                         radmmm_stream_t stream) {
  RADMMM_REQUIRE(src && offsets && lens && scratch, "collate_unpack_pad: null pointer");
  RADMMM_REQUIRE(B > 0 && B <= 65535 && Smax > n_fft / 2 && n_fft > 0 && n_fft % 4 == 0,
                 "collate_unpack_pad: bad dims (need n_fft %% 4 == 0, Smax > n_fft/2, B <= 65535)");
  RADMMM_REQUIRE(radmmm::aligned16(src) && radmmm::aligned16(scratch), "collate_unpack_pad: src/scratch must be 16B aligned");
  RADMMM_REQUIRE((long long)Smax + n_fft < INT_MAX - 4, "collate_unpack_pad: Smax too large");
  const int pitch = (int)r4((long long)Smax + n_fft);
  hipLaunchKernelGGL(unpack_pad_kernel, dim3((pitch / 4 + 255) / 256, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     src, src_int16, reinterpret_cast<const long long*>(offsets), lens, scratch, audio, n_fft / 2, pitch,
                     Smax, scale);
  return radmmm::check_launch("collate_unpack_pad");
}

extern "C" int radmmm_collate_mel(const float* basis, const float* mel_basis, const int32_t* frames, float* mel,
                                  float* energy, float* scratch, int B, int Smax, int n_fft, int hop, int n_mel,
                                  float clip, int scaled, radmmm_stream_t stream) {
  RADMMM_REQUIRE(basis && mel_basis && frames && mel && scratch, "collate_mel: null pointer");
  RADMMM_REQUIRE(B > 0 && B <= 65535 && Smax > n_fft / 2 && n_fft > 0 && n_fft % 4 == 0 && hop > 0 && hop % 4 == 0 && n_mel > 0,
                 "collate_mel: bad dims (need n_fft %% 4 == 0, hop %% 4 == 0, Smax > n_fft/2, B <= 65535)");
  RADMMM_REQUIRE(radmmm::aligned16(basis) && radmmm::aligned16(scratch), "collate_mel: basis/scratch must be 16B aligned");
  const StftLayout L = stft_layout(B, Smax, n_fft, hop, n_mel);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* xpad = scratch + L.off_xpad;
  float* spec = scratch + L.off_spec;
  float* mag = scratch + L.off_mag;
  float* melb = scratch + L.off_melb;
  float* melT = scratch + L.off_melT;
  hipLaunchKernelGGL(pad_cols_kernel, dim3(grid_for((long long)n_mel * L.ldm)), dim3(256), 0, s, mel_basis,
                     L.cutoff, melb, L.ldm, n_mel, L.cutoff);
  int rc = radmmm::check_launch("collate_mel: pad");
  if (rc) return rc;
  radmmm_rowgemm_desc d = {};
  d.A = xpad; d.lda = hop; d.a_item_stride = L.pitch;
  d.B = basis; d.ldb = n_fft; d.b_tap_stride = 0; d.b_layout = 0;
  d.C = spec; d.ldc = L.lds;
  d.M = B * L.F; d.N = 2 * L.cutoff; d.K = n_fft;
  d.taps = 1; d.dil = 1; d.sign = 1; d.T = L.F; d.ratio_taps = 1; d.ratio_dil = 1;
  rc = radmmm_rowgemm_f32(&d, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(magnitude_kernel, dim3(grid_for((long long)B * L.F * L.ldm)), dim3(256), 0, s, spec,
                     L.lds, mag, L.ldm, (long long)B * L.F, L.cutoff);
  radmmm_rowgemm_desc m = {};
  m.A = mag; m.lda = L.ldm;
  m.B = melb; m.ldb = L.ldm; m.b_layout = 0;
  m.C = melT; m.ldc = L.ldt;
  m.M = B * L.F; m.N = n_mel; m.K = L.cutoff;
  m.taps = 1; m.dil = 1; m.sign = 1; m.T = L.F; m.ratio_taps = 1; m.ratio_dil = 1;
  rc = radmmm_rowgemm_f32(&m, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(finish_kernel, dim3((L.F + 255) / 256, B), dim3(256), 0, s, melT, L.ldt, frames, mel, energy, L.F,
                     n_mel, clip, scaled);
  return radmmm::check_launch("collate_mel");
}

extern "C" int radmmm_collate_tracks(const float* f0_packed, const float* p_voiced_packed, const float* voiced_mask_packed,
                                     const int32_t* ids_packed, const int64_t* frame_offsets, const int64_t* token_offsets,
                                     const int32_t* frames, const int32_t* in_lens, float* f0, float* p_voiced,
                                     float* voiced_mask, int64_t* text, int32_t* scan, const int64_t* meta_src,
                                     int64_t* meta_dst, int n_meta, int B, int Tmax, int Lmax, float f0_min, int use_log_f0,
                                     int distance_tx, radmmm_stream_t stream) {
  RADMMM_REQUIRE(frame_offsets && frames, "collate_tracks: null pointer");
  RADMMM_REQUIRE(B > 0 && B <= 65535 && Tmax > 0 && Lmax >= 0 && n_meta >= 0, "collate_tracks: bad dims");
  RADMMM_REQUIRE((f0 == nullptr) == (f0_packed == nullptr) && (p_voiced == nullptr) == (p_voiced_packed == nullptr) &&
                     (voiced_mask == nullptr) == (voiced_mask_packed == nullptr),
                 "collate_tracks: a track needs both its packed input and its output");
  RADMMM_REQUIRE(!text || (ids_packed && token_offsets && in_lens && Lmax > 0), "collate_tracks: text needs ids, offsets, lengths");
  RADMMM_REQUIRE(!(f0 && distance_tx) || scan, "collate_tracks: the distance transform needs the scan scratch [B][Tmax]");
  RADMMM_REQUIRE(n_meta == 0 || (meta_src && meta_dst), "collate_tracks: meta copy needs both pointers");
  hipLaunchKernelGGL(tracks_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), f0_packed, p_voiced_packed,
                     voiced_mask_packed, ids_packed, reinterpret_cast<const long long*>(frame_offsets),
                     reinterpret_cast<const long long*>(token_offsets), frames, in_lens, f0, p_voiced, voiced_mask,
                     reinterpret_cast<long long*>(text), scan, reinterpret_cast<const long long*>(meta_src),
                     reinterpret_cast<long long*>(meta_dst), n_meta, Tmax, Lmax, f0_min, use_log_f0, distance_tx);
  return radmmm::check_launch("collate_tracks");
}
