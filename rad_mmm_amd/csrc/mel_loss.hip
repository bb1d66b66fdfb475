// Differentiable log-mel and the mel L1 loss (mel_loss.py: mel_spectrogram, MelSpectrogramLoss) on gfx950: what surrounds
// the row GEMMs (frames x forward_basis, mag x mel_basis^T forward; dmelp x mel_basis, dspec x forward_basis backward).
//
// Layout.  A signal is [B][ldx] fp32 with lens[b] samples in item b (an int32 device array; NULL: S everywhere), read
// clamped to [1, S].  TacotronSTFT.mel_spectrogram reflect-pads an item by h = n_fft / 2 about 0 and about lens[b] - 1 and
// cuts 1 + lens[b] / hop frames of n_fft samples (the window lives in the basis); F = 1 + S / hop rows per item,
// r = b*F + f.  Every reflected index is clamped into [0, lens[b] - 1], so that no value of lens reaches outside an item.
// spec is [B*F][lds], re in columns [0, cutoff), im in [cutoff, 2 cutoff), cutoff = n_fft / 2 + 1; mag is [B*F][ldm] and
// melp [B*F][ldn].  Mels in the reference layout are [B][n_mel][Ft].  n[b] = min(item frames, Ft, frames[b] clamped into
// [0, min(F, Ft)]) frames of item b enter the loss.
//
//   radmmm_melloss_frame    signal -> frame matrix, zeros in rows past an item's frames
//   radmmm_melloss_mag      spec -> sqrt(re^2 + im^2), zeros in the pad columns and in rows past an item's frames
//   radmmm_melloss_terms    melp -> log(max(melp, clip)): the mel in the reference layout and / or per-row sum_c |mel - target|
//   radmmm_melloss_finish   partials -> loss and the normaliser sum_b n[b], one workgroup, fp64
//   radmmm_melloss_bwd      gradient of melp, from the loss (sign recomputed from melp and target) or from an upstream dmel
//   radmmm_melloss_dspec    dmag -> gradient of the spectrum (0 where mag == 0)
//   radmmm_melloss_unframe  dA -> dx: the adjoint of frame in gather form
// Every reduction has a fixed order and there are no atomics: equal inputs give equal bits.
#include "common.h"

namespace {

using radmmm::block_sum_f64;
using radmmm::grid_for;
using radmmm::ST;

constexpr int kRowsPerBlock = 4;   // one wave per row, four rows per workgroup
constexpr int kFinishThreads = 1024;
constexpr int kTF = 32;            // frames of a transposing tile
constexpr int kTC = 64;            // channels of a transposing tile: lane l of a row's wave meets channels l, l + 64, ...
constexpr int kTLd = kTF + 1;      // LDS row stride: lanes over channels fall on distinct banks

__device__ __forceinline__ int item_len(const int32_t* lens, int b, int S) {
  if (!lens) return S;
  const int n = lens[b];
  return n < 1 ? 1 : (n > S ? S : n);
}
// frames of an item: 1 + len / hop <= F = 1 + S / hop
__device__ __forceinline__ int item_frames(const int32_t* lens, int b, int S, int hop) { return 1 + item_len(lens, b, S) / hop; }
// frames of an item that enter the loss
__device__ __forceinline__ int loss_frames(const int32_t* lens, const int32_t* frames, int b, int S, int F, int Ft, int hop) {
  int n = item_frames(lens, b, S, hop);
  const int cap = F < Ft ? F : Ft;
  n = n < cap ? n : cap;
  if (frames) {
    int q = frames[b];
    q = q < 0 ? 0 : (q > cap ? cap : q);
    n = n < q ? n : q;
  }
  return n;
}

// x[b][reflect(f*hop + j - h)] -> A[(b*F + f)*n_fft + j]; four columns per thread
__global__ void __launch_bounds__(256) frame_kernel(const float* __restrict__ x, int ldx, const int32_t* __restrict__ lens,
                                                    float* __restrict__ A, long long rows, int S, int F, int n_fft, int hop) {
  const int q = n_fft >> 2, h = n_fft >> 1;
  const long long total = rows * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int j0 = (int)(i - r * q) * 4;
    const int b = (int)(r / F), f = (int)(r - (long long)b * F);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int len = item_len(lens, b, S);
    if (f < 1 + len / hop) {
      const float* xb = x + (long long)b * ldx;
      const int p0 = f * hop + j0 - h;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int p = p0 + e;
        p = p < 0 ? -p : p;
        p = p > len - 1 ? 2 * (len - 1) - p : p;
        p = p < 0 ? 0 : (p > len - 1 ? len - 1 : p);   // an item of len <= h: unspecified but inside the item
        v[e] = xb[p];
      }
    }
    *reinterpret_cast<float4*>(A + r * n_fft + j0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// mag[r][k] = sqrt(re^2 + im^2); four columns per thread, 0 for cutoff <= k < ldm and in rows past an item's frames
__global__ void __launch_bounds__(256) mag_kernel(const float* __restrict__ spec, int lds, const int32_t* __restrict__ lens,
                                                  float* __restrict__ mag, int ldm, long long rows, int S, int F, int hop,
                                                  int cutoff) {
  const int q = ldm >> 2;
  const long long total = rows * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int k0 = (int)(i - r * q) * 4;
    const int b = (int)(r / F), f = (int)(r - (long long)b * F);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (f < item_frames(lens, b, S, hop)) {
      const float* p = spec + r * lds;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (k0 + e < cutoff) {
          const float re = p[k0 + e], im = p[cutoff + k0 + e];
          v[e] = sqrtf(re * re + im * im);
        }
      }
    }
    *reinterpret_cast<float4*>(mag + r * ldm + k0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// log(max(melp, clip)), taken in double and rounded once: the correctly rounded fp32 log (logf lies more than one ulp off in places), and
// the same bits wherever the forward and the backward form it
__device__ __forceinline__ float log_mel(float melp, float clip) { return (float)log((double)fmaxf(melp, clip)); }

// src [B][n_mel][ld] (a mel in the reference layout) -> tile[c - c0][f - f0] for c < n_mel, f < nf; 0 elsewhere
__device__ __forceinline__ void load_tile(float (*tile)[kTLd], const float* __restrict__ src, int ld, int b, int n_mel, int c0,
                                          int f0, int nf) {
  const int fl = threadIdx.x & (kTF - 1), f = f0 + fl;
  for (int cl = threadIdx.x / kTF; cl < kTC; cl += 256 / kTF) {
    const int c = c0 + cl;
    tile[cl][fl] = (c < n_mel && f < nf) ? src[((long long)b * n_mel + c) * ld + f] : 0.f;
  }
}

// One workgroup: kTF frames of one item, the channels in tiles of kTC.  mel_out[b][c][f] = log(max(melp, clip)) for
// f < item frames, 0 up to F.  part[r] = sum_c |mel - target[b][c][f]| for f < n[b], else 0: lane l of the row's wave adds
// channels l, l + 64, ... in order, then the wave's xor butterfly adds the 64 lane sums.
__global__ void __launch_bounds__(256) terms_kernel(const float* __restrict__ melp, int ldn, const int32_t* __restrict__ lens,
                                                    const int32_t* __restrict__ frames, const float* __restrict__ target, int Ft,
                                                    float* __restrict__ mel_out, float* __restrict__ part, int S, int F, int hop,
                                                    int n_mel, float clip, int tiles_f) {
  __shared__ float sm[kTC][kTLd];
  __shared__ float st[kTC][kTLd];
  const int b = blockIdx.x / tiles_f, f0 = (blockIdx.x - b * tiles_f) * kTF;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nfx = item_frames(lens, b, S, hop);
  const int nl = target ? loss_frames(lens, frames, b, S, F, Ft, hop) : 0;
  constexpr int kPer = kTF / 4;    // rows of a wave
  float acc[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) acc[i] = 0.f;
  for (int c0 = 0; c0 < n_mel; c0 += kTC) {
    const int c = c0 + lane;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int fl = w * kPer + i, f = f0 + fl;
      sm[lane][fl] = (c < n_mel && f < nfx) ? log_mel(melp[((long long)b * F + f) * ldn + c], clip) : 0.f;
    }
    if (target) load_tile(st, target, Ft, b, n_mel, c0, f0, nl);
    __syncthreads();
    if (mel_out) {
      const int fl = threadIdx.x & (kTF - 1), f = f0 + fl;
      for (int cl = threadIdx.x / kTF; cl < kTC; cl += 256 / kTF) {
        if (c0 + cl < n_mel && f < F) mel_out[((long long)b * n_mel + c0 + cl) * F + f] = sm[cl][fl];
      }
    }
    if (target && c < n_mel) {
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int fl = w * kPer + i;
        if (f0 + fl < nl) acc[i] += fabsf(sm[lane][fl] - st[lane][fl]);
      }
    }
    __syncthreads();
  }
  if (part) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int f = f0 + w * kPer + i;
      const float s = radmmm::wave_sum(acc[i]);
      if (lane == 0 && f < F) part[(long long)b * F + f] = s;
    }
  }
}

// one workgroup: norm[0] = sum_b n[b], out[0] = sum over the rows f < n[b] of part / (n_mel * norm[0]); 0 when no frame counts
__global__ void __launch_bounds__(kFinishThreads) finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ lens,
                                                                const int32_t* __restrict__ frames, float* __restrict__ out,
                                                                double* __restrict__ norm, int B, int S, int F, int Ft, int hop,
                                                                int n_mel) {
  __shared__ double sh[kFinishThreads];
  const long long rows = (long long)B * F;
  double sum = 0.0, cnt = 0.0;
  for (long long r = threadIdx.x; r < rows; r += kFinishThreads) {
    const int b = (int)(r / F), f = (int)(r - (long long)b * F);
    if (f < loss_frames(lens, frames, b, S, F, Ft, hop)) sum += (double)part[r];
  }
  for (int b = threadIdx.x; b < B; b += kFinishThreads) cnt += (double)loss_frames(lens, frames, b, S, F, Ft, hop);
  sum = block_sum_f64<kFinishThreads>(sum, sh);
  cnt = block_sum_f64<kFinishThreads>(cnt, sh);
  if (threadIdx.x == 0) {
    out[0] = cnt > 0.0 ? (float)(sum / ((double)n_mel * cnt)) : 0.f;
    norm[0] = cnt;
  }
}

// dmelp[r][c]: with a target, g[0] * sign(mel - target) / (n_mel * norm[0]) / melp for f < n[b]; with an upstream dmel
// [B][n_mel][F], dmel / melp for f < item frames; 0 where melp < clip, in the other rows and in columns n_mel <= c < ldn
__global__ void __launch_bounds__(256) bwd_kernel(const float* __restrict__ melp, int ldn, const int32_t* __restrict__ lens,
                                                  const int32_t* __restrict__ frames, const float* __restrict__ target, int Ft,
                                                  const double* __restrict__ norm, const float* __restrict__ g,
                                                  const float* __restrict__ dmel, float* __restrict__ dmelp, int S, int F, int hop,
                                                  int n_mel, float clip, int tiles_f) {
  __shared__ float st[kTC][kTLd];
  const int b = blockIdx.x / tiles_f, f0 = (blockIdx.x - b * tiles_f) * kTF;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nf = target ? loss_frames(lens, frames, b, S, F, Ft, hop) : item_frames(lens, b, S, hop);
  float coef = 0.f;
  if (target) {
    const double cnt = norm[0];
    coef = cnt > 0.0 ? (float)((double)g[0] / ((double)n_mel * cnt)) : 0.f;
  }
  constexpr int kPer = kTF / 4;
  for (int c0 = 0; c0 < ldn; c0 += kTC) {
    load_tile(st, target ? target : dmel, target ? Ft : F, b, n_mel, c0, f0, nf);
    __syncthreads();
    const int c = c0 + lane;
    if (c < ldn) {
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int fl = w * kPer + i, f = f0 + fl;
        if (f >= F) continue;
        const long long at = ((long long)b * F + f) * ldn + c;
        float v = 0.f;
        if (c < n_mel && f < nf) {
          const float m = melp[at];
          if (m >= clip) {
            if (target) {
              const float d = log_mel(m, clip) - st[lane][fl];
              v = (d > 0.f ? coef : (d < 0.f ? -coef : 0.f)) / m;
            } else {
              v = st[lane][fl] / m;
            }
          }
        }
        dmelp[at] = v;
      }
    }
    __syncthreads();
  }
}

// dspec[r] = (dmag * re / mag | dmag * im / mag), mag = sqrt(re^2 + im^2) as mag_kernel forms it; 0 where mag == 0, in
// rows past an item's frames and in columns 2 cutoff <= c < lds.  One wave per row.
__global__ void __launch_bounds__(64 * kRowsPerBlock) dspec_kernel(const float* __restrict__ dmag, int ldm,
                                                                   const float* __restrict__ spec, int lds,
                                                                   const int32_t* __restrict__ lens, float* __restrict__ dspec,
                                                                   long long rows, int S, int F, int hop, int cutoff) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / F), f = (int)(r - (long long)b * F);
  float* o = dspec + r * lds;
  if (f >= item_frames(lens, b, S, hop)) {
    for (int c = lane; c < lds; c += 64) o[c] = 0.f;
    return;
  }
  const float* p = spec + r * lds;
  const float* d = dmag + r * ldm;
  for (int k = lane; k < cutoff; k += 64) {
    const float re = p[k], im = p[cutoff + k];
    const float m = sqrtf(re * re + im * im);
    const float s = m > 0.f ? d[k] / m : 0.f;
    o[k] = m > 0.f ? s * re : 0.f;
    o[cutoff + k] = m > 0.f ? s * im : 0.f;
  }
  for (int c = 2 * cutoff + lane; c < lds; c += 64) o[c] = 0.f;
}

// sum of dA over the frames f < nf that hold padded position P (column P - f*hop in [0, n_fft)), f ascending
__device__ __forceinline__ float gather_position(const float* __restrict__ dAb, int n_fft, int P, int nf, int hop) {
  if (P < 0) return 0.f;
  int f_hi = P / hop;
  if (f_hi > nf - 1) f_hi = nf - 1;
  const int lo = P - n_fft + 1;
  const int f_lo = lo > 0 ? (lo + hop - 1) / hop : 0;
  float s = 0.f;
  for (int f = f_lo; f <= f_hi; ++f) s += dAb[(long long)f * n_fft + (P - f * hop)];
  return s;
}

// dx[b][s], s < len: own position s + h, then the left mirror h - s (1 <= s <= h), then the right mirror
// h + 2(len-1) - s (len-1-h <= s <= len-2); a sample has both when len = h + 1.  s >= len: 0 (left alone with accum).
__global__ void __launch_bounds__(256) unframe_kernel(const float* __restrict__ dA, const int32_t* __restrict__ lens,
                                                      float* __restrict__ dx, int lddx, int B, int S, int F, int n_fft, int hop,
                                                      int accum) {
  const int h = n_fft >> 1;
  const long long total = (long long)B * S;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / S), s = (int)(i - (long long)b * S);
    const int len = item_len(lens, b, S);
    float* o = dx + (long long)b * lddx + s;
    if (s >= len) {
      if (!accum) *o = 0.f;
      continue;
    }
    const int nf = 1 + len / hop;
    const float* dAb = dA + (long long)b * F * n_fft;
    float g = gather_position(dAb, n_fft, s + h, nf, hop);
    if (s >= 1 && s <= h) g += gather_position(dAb, n_fft, h - s, nf, hop);
    if (s >= len - 1 - h && s <= len - 2) g += gather_position(dAb, n_fft, h + 2 * (len - 1) - s, nf, hop);
    *o = accum ? *o + g : g;
  }
}

// B items of S samples, F = 1 + S / hop rows each
int check_rows(const char* who, int B, int S, int F, int hop) {
  RADMMM_REQUIRE(B > 0 && S > 0 && hop >= 1 && F >= 1, "%s: bad dims (B=%d S=%d F=%d hop=%d)", who, B, S, F, hop);
  RADMMM_REQUIRE(F == 1 + S / hop, "%s: F=%d is not 1 + S / hop = %d", who, F, 1 + S / hop);
  return 0;
}

int check_geometry(const char* who, int B, int S, int F, int n_fft, int hop) {
  RADMMM_REQUIRE(n_fft >= 4 && n_fft % 4 == 0, "%s: n_fft=%d must be a positive multiple of 4", who, n_fft);
  if (int rc = check_rows(who, B, S, F, hop)) return rc;
  RADMMM_REQUIRE(S > n_fft / 2, "%s: S=%d cannot be reflect-padded by n_fft/2=%d", who, S, n_fft / 2);
  RADMMM_REQUIRE((long long)B * F * n_fft * 4 < 0x7fffffffLL, "%s: the frame matrix exceeds 2 GiB", who);
  return 0;
}

int check_spec(const char* who, int B, int F, int cutoff, int lds, int ldm) {
  RADMMM_REQUIRE(cutoff > 0, "%s: bad dims (cutoff=%d)", who, cutoff);
  RADMMM_REQUIRE(lds % 4 == 0 && lds >= 2 * cutoff, "%s: lds=%d must be a multiple of 4 and >= 2 * cutoff=%d", who, lds, 2 * cutoff);
  RADMMM_REQUIRE(ldm % 4 == 0 && ldm >= cutoff, "%s: ldm=%d must be a multiple of 4 and >= cutoff=%d", who, ldm, cutoff);
  RADMMM_REQUIRE((long long)B * F * lds * 4 < 0x7fffffffLL, "%s: the spectrum exceeds 2 GiB", who);
  return 0;
}

int check_mel(const char* who, int B, int F, int n_mel, int ldn) {
  RADMMM_REQUIRE(n_mel > 0, "%s: bad dims (n_mel=%d)", who, n_mel);
  RADMMM_REQUIRE(ldn % 4 == 0 && ldn >= n_mel, "%s: ldn=%d must be a multiple of 4 and >= n_mel=%d", who, ldn, n_mel);
  RADMMM_REQUIRE((long long)B * F * ldn * 4 < 0x7fffffffLL, "%s: the mel matrix exceeds 2 GiB", who);
  return 0;
}

}  // namespace

extern "C" int radmmm_melloss_frame(const float* x, int ldx, const int32_t* lens, float* A, int B, int S, int F, int n_fft,
                                    int hop, radmmm_stream_t stream) {
  RADMMM_REQUIRE(x && A, "melloss_frame: null pointer");
  if (int rc = check_geometry("melloss_frame", B, S, F, n_fft, hop)) return rc;
  RADMMM_REQUIRE(ldx >= S, "melloss_frame: ldx=%d < S=%d", ldx, S);
  RADMMM_REQUIRE(radmmm::aligned16(A), "melloss_frame: A must be 16B aligned");
  const long long rows = (long long)B * F;
  hipLaunchKernelGGL(frame_kernel, dim3(grid_for(rows * (n_fft / 4), 256)), dim3(256), 0, ST(stream), x, ldx, lens, A, rows, S, F,
                     n_fft, hop);
  return radmmm::check_launch("melloss_frame");
}

extern "C" int radmmm_melloss_mag(const float* spec, int lds, const int32_t* lens, float* mag, int ldm, int B, int S, int F,
                                  int hop, int cutoff, radmmm_stream_t stream) {
  RADMMM_REQUIRE(spec && mag, "melloss_mag: null pointer");
  if (int rc = check_rows("melloss_mag", B, S, F, hop)) return rc;
  if (int rc = check_spec("melloss_mag", B, F, cutoff, lds, ldm)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(mag), "melloss_mag: mag must be 16B aligned");
  const long long rows = (long long)B * F;
  hipLaunchKernelGGL(mag_kernel, dim3(grid_for(rows * (ldm / 4), 256)), dim3(256), 0, ST(stream), spec, lds, lens, mag, ldm, rows,
                     S, F, hop, cutoff);
  return radmmm::check_launch("melloss_mag");
}

extern "C" int radmmm_melloss_terms(const float* melp, int ldn, const int32_t* lens, const int32_t* frames, const float* target,
                                    int Ft, float* mel_out, float* part, int B, int S, int F, int hop, int n_mel, float clip,
                                    radmmm_stream_t stream) {
  RADMMM_REQUIRE(melp && (mel_out || part), "melloss_terms: null pointer");
  RADMMM_REQUIRE((target != nullptr) == (part != nullptr), "melloss_terms: target and part come together");
  if (int rc = check_rows("melloss_terms", B, S, F, hop)) return rc;
  if (int rc = check_mel("melloss_terms", B, F, n_mel, ldn)) return rc;
  RADMMM_REQUIRE(!target || Ft >= 1, "melloss_terms: Ft=%d", Ft);
  RADMMM_REQUIRE(clip > 0.f, "melloss_terms: clip must be positive");
  const int tiles_f = (F + kTF - 1) / kTF;
  RADMMM_REQUIRE((long long)B * tiles_f < 0x7fffffffLL, "melloss_terms: too many tiles");
  hipLaunchKernelGGL(terms_kernel, dim3((unsigned)(B * tiles_f)), dim3(256), 0, ST(stream), melp, ldn, lens, frames, target, Ft,
                     mel_out, part, S, F, hop, n_mel, clip, tiles_f);
  return radmmm::check_launch("melloss_terms");
}

extern "C" int radmmm_melloss_finish(const float* part, const int32_t* lens, const int32_t* frames, float* out, double* norm,
                                     int B, int S, int F, int Ft, int hop, int n_mel, radmmm_stream_t stream) {
  RADMMM_REQUIRE(part && out && norm, "melloss_finish: null pointer");
  if (int rc = check_rows("melloss_finish", B, S, F, hop)) return rc;
  RADMMM_REQUIRE(Ft >= 1 && n_mel > 0, "melloss_finish: bad dims (Ft=%d n_mel=%d)", Ft, n_mel);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kFinishThreads), 0, ST(stream), part, lens, frames, out, norm, B, S, F, Ft, hop,
                     n_mel);
  return radmmm::check_launch("melloss_finish");
}

extern "C" int radmmm_melloss_bwd(const float* melp, int ldn, const int32_t* lens, const int32_t* frames, const float* target,
                                  int Ft, const double* norm, const float* g, const float* dmel, float* dmelp, int B, int S,
                                  int F, int hop, int n_mel, float clip, radmmm_stream_t stream) {
  RADMMM_REQUIRE(melp && dmelp, "melloss_bwd: null pointer");
  RADMMM_REQUIRE((target != nullptr) != (dmel != nullptr), "melloss_bwd: exactly one of target and dmel");
  RADMMM_REQUIRE(!target || (norm && g), "melloss_bwd: null pointer");
  if (int rc = check_rows("melloss_bwd", B, S, F, hop)) return rc;
  if (int rc = check_mel("melloss_bwd", B, F, n_mel, ldn)) return rc;
  RADMMM_REQUIRE(!target || Ft >= 1, "melloss_bwd: Ft=%d", Ft);
  RADMMM_REQUIRE(clip > 0.f, "melloss_bwd: clip must be positive");
  const int tiles_f = (F + kTF - 1) / kTF;
  RADMMM_REQUIRE((long long)B * tiles_f < 0x7fffffffLL, "melloss_bwd: too many tiles");
  hipLaunchKernelGGL(bwd_kernel, dim3((unsigned)(B * tiles_f)), dim3(256), 0, ST(stream), melp, ldn, lens, frames, target, Ft, norm,
                     g, dmel, dmelp, S, F, hop, n_mel, clip, tiles_f);
  return radmmm::check_launch("melloss_bwd");
}

extern "C" int radmmm_melloss_dspec(const float* dmag, int ldm, const float* spec, int lds, const int32_t* lens, float* dspec,
                                    int B, int S, int F, int hop, int cutoff, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dmag && spec && dspec, "melloss_dspec: null pointer");
  if (int rc = check_rows("melloss_dspec", B, S, F, hop)) return rc;
  if (int rc = check_spec("melloss_dspec", B, F, cutoff, lds, ldm)) return rc;
  const long long rows = (long long)B * F;
  hipLaunchKernelGGL(dspec_kernel, dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(64 * kRowsPerBlock), 0,
                     ST(stream), dmag, ldm, spec, lds, lens, dspec, rows, S, F, hop, cutoff);
  return radmmm::check_launch("melloss_dspec");
}

extern "C" int radmmm_melloss_unframe(const float* dA, const int32_t* lens, float* dx, int lddx, int B, int S, int F, int n_fft,
                                      int hop, int accum, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dA && dx, "melloss_unframe: null pointer");
  if (int rc = check_geometry("melloss_unframe", B, S, F, n_fft, hop)) return rc;
  RADMMM_REQUIRE(lddx >= S, "melloss_unframe: lddx=%d < S=%d", lddx, S);
  hipLaunchKernelGGL(unframe_kernel, dim3(grid_for((long long)B * S, 256)), dim3(256), 0, ST(stream), dA, lens, dx, lddx, B, S, F,
                     n_fft, hop, accum);
  return radmmm::check_launch("melloss_unframe");
}
