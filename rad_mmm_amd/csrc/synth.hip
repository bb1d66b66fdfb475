// Synthesis glue on gfx950: what joins the duration predictor, the frame-rate attribute predictors and the flow
// decoder's inverse in TTSModel.sample_full / reconstruct_from_batch_attributes (tts_lightning_modules.py:286-437).
// The reference does this in Python per utterance and per token; here each step is one launch over the padded batch:
//   radmmm_synth_durations  clamp(round(d), 1) * mask -> int32 durations, inclusive prefix sums and frame counts
//   radmmm_synth_regulate   LengthRegulator (common.py:208-237) as a gather into channels-last frame rows
//   radmmm_synth_f0_stats   per-workgroup fp64 sums of the voiced frames' f0 (the "shift stats", :367-376)
//   radmmm_synth_f0_apply   voiced gate, f0 * voiced, shift-stats renormalisation and the length mask of f0 / energy
// No floating-point atomics: every sum has a fixed order, so the results are bitwise repeatable.
#include <math.h>

#include "common.h"

namespace {

using radmmm::ST;

constexpr int SYN_BLOCK = 256;
constexpr int SYN_MAX_DUR = 65536;      // frames per token: guards the prefix sums against absurd / non-finite predictions
constexpr int SYN_MAX_TT = 32767;       // SYN_MAX_TT * SYN_MAX_DUR < 2^31: the prefix sums fit int32
constexpr int REG_FRAMES = 16;          // frames per regulate workgroup
constexpr int REG_MAX_TT = 16384;       // prefix sums staged in LDS (64 KiB)
constexpr int F0_MAX_PARTS = 1024;

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// torch.sigmoid(v) > 0.5 as the reference evaluates it; `v > 0` differs where 1 / (1 + exp(-v)) rounds to 0.5
__device__ __forceinline__ bool voiced_of(float v) { return 1.f / (1.f + expf(-v)) > 0.5f; }

// One workgroup per utterance, the tokens in chunks of SYN_BLOCK: per chunk a wave scan, the wave totals through LDS and
// the running carry of the earlier chunks.
__global__ __launch_bounds__(SYN_BLOCK) void durations_kernel(const float* __restrict__ x, long long item_stride, int Tt,
                                                              const int32_t* __restrict__ text_lens, int integer_mode,
                                                              int32_t* __restrict__ dur, int32_t* __restrict__ cum,
                                                              int32_t* __restrict__ out_lens) {
  __shared__ int wsum[SYN_BLOCK / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* xb = x + (long long)b * item_stride;
  int len = text_lens ? text_lens[b] : Tt;
  len = len < 0 ? 0 : (len > Tt ? Tt : len);
  int carry = 0;
  for (int base = 0; base < Tt; base += SYN_BLOCK) {
    const int t = base + tid;
    int d = 0;
    if (t < len) {
      float v = xb[t];
      // fmaxf / fminf return the non-NaN operand: NaN becomes the lower bound
      v = integer_mode ? fmaxf(v, 0.f) : fmaxf(rintf(v), 1.f);
      d = (int)fminf(v, (float)SYN_MAX_DUR);
    }
    const int s = wave_incl_scan(d, lane);
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    int off = carry, total = 0;
#pragma unroll
    for (int i = 0; i < SYN_BLOCK / 64; ++i) {
      off += i < w ? wsum[i] : 0;
      total += wsum[i];
    }
    __syncthreads();
    if (t < Tt) {
      dur[(long long)b * Tt + t] = d;
      cum[(long long)b * Tt + t] = off + s;
    }
    carry += total;
  }
  if (tid == 0) out_lens[b] = carry;
}

// rows[(b * Tmax + t) * ldc + c] = txt[b * item_stride + j * row_stride + c] for t < out_lens[b] and c < C, where token j
// covers frame t (the first j with cum[b, j] > t); zeros elsewhere.  Frame-major grid (REG_FRAMES frames of one utterance
// per workgroup), one float4 per thread and step.
__global__ __launch_bounds__(SYN_BLOCK) void regulate_kernel(const float* __restrict__ txt, long long item_stride,
                                                             int row_stride, int Tt, int C,
                                                             const int32_t* __restrict__ cum,
                                                             const int32_t* __restrict__ out_lens,
                                                             float* __restrict__ rows, int ldc, int Tmax) {
  extern __shared__ int lds[];
  int* scum = lds;
  int* tok = lds + Tt;
  const int b = blockIdx.y, t0 = blockIdx.x * REG_FRAMES;
  const int32_t* cb = cum + (long long)b * Tt;
  for (int i = threadIdx.x; i < Tt; i += blockDim.x) scum[i] = cb[i];
  __syncthreads();
  if (threadIdx.x < REG_FRAMES) {
    int len = out_lens[b];
    len = len < Tmax ? len : Tmax;
    const int t = t0 + threadIdx.x;
    int j = -1;
    if (t < len) {
      int lo = 0, hi = Tt;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (scum[mid] <= t) lo = mid + 1;
        else hi = mid;
      }
      j = lo < Tt ? lo : Tt - 1;
    }
    tok[threadIdx.x] = j;
  }
  __syncthreads();
  const int q = ldc >> 2, cq = C >> 2;
  const int nf = Tmax - t0 < REG_FRAMES ? Tmax - t0 : REG_FRAMES;
  const float* xb = txt + (long long)b * item_stride;
  float* ob = rows + ((long long)b * Tmax + t0) * ldc;
  for (int i = threadIdx.x; i < nf * q; i += blockDim.x) {
    const int f = i / q, c4 = i - f * q;
    const int j = tok[f];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j >= 0 && c4 < cq) v = *reinterpret_cast<const float4*>(xb + (long long)j * row_stride + c4 * 4);
    *reinterpret_cast<float4*>(ob + (long long)f * ldc + c4 * 4) = v;
  }
}

// part[k * nparts + blockIdx.x], k = 0, 1, 2: count, sum and sum of squares (fp64) of f0 over the voiced frames
// t < lens[b] that this workgroup's grid-stride share covers
__global__ __launch_bounds__(SYN_BLOCK) void f0_stats_kernel(const float* __restrict__ f0, long long f0s,
                                                             const float* __restrict__ vl, long long vs,
                                                             const int32_t* __restrict__ lens, int B, int T,
                                                             double* __restrict__ part, int nparts) {
  __shared__ double sh[3][SYN_BLOCK / 64];
  double n = 0.0, s = 0.0, ss = 0.0;
  const long long total = (long long)B * T;
  for (long long i = blockIdx.x * (long long)SYN_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * SYN_BLOCK) {
    const int b = (int)(i / T), t = (int)(i - (long long)b * T);
    if (t < lens[b] && voiced_of(vl[b * vs + t])) {
      const double f = (double)f0[b * f0s + t];
      n += 1.0;
      s += f;
      ss += f * f;
    }
  }
  n = wave_sum_d(n);
  s = wave_sum_d(s);
  ss = wave_sum_d(ss);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    sh[0][w] = n;
    sh[1][w] = s;
    sh[2][w] = ss;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double a = 0.0;
    for (int i = 0; i < SYN_BLOCK / 64; ++i) a += sh[threadIdx.x][i];
    part[threadIdx.x * nparts + blockIdx.x] = a;
  }
}

// out[b, t] for t < T (contiguous [B, T]): voiced = sigmoid(v) > 0.5 and t < lens[b]; f0 * voiced, renormalised on the voiced
// frames to (f0 - mu) / sigma * f0_std[b] + f0_mean[b] when part != NULL and at least 2 voiced frames with sigma > 0 exist
// (mu and the unbiased sigma from the partial sums, reduced by every workgroup in the same order); energy masked to lens[b].
__global__ __launch_bounds__(SYN_BLOCK) void f0_apply_kernel(const float* __restrict__ f0, long long f0s,
                                                             const float* __restrict__ vl, long long vs,
                                                             const float* __restrict__ en, long long ens,
                                                             const int32_t* __restrict__ lens, int B, int T,
                                                             const double* __restrict__ part, int nparts,
                                                             const float* __restrict__ f0_mean,
                                                             const float* __restrict__ f0_std, float* __restrict__ f0o,
                                                             float* __restrict__ eno, float* __restrict__ vo) {
  __shared__ float stat[2];
  __shared__ int shift;
  if (threadIdx.x < 64) {
    double n = 0.0, s = 0.0, ss = 0.0;
    if (part) {
      for (int k = threadIdx.x; k < nparts; k += 64) {
        n += part[k];
        s += part[nparts + k];
        ss += part[2 * nparts + k];
      }
    }
    n = wave_sum_d(n);
    s = wave_sum_d(s);
    ss = wave_sum_d(ss);
    if (threadIdx.x == 0) {
      int on = 0;
      if (part && n >= 2.0) {
        const double mu = s / n;
        const double var = (ss - s * mu) / (n - 1.0);
        const double sig = var > 0.0 ? sqrt(var) : 0.0;
        on = sig > 0.0;
        stat[0] = (float)mu;
        stat[1] = (float)sig;
      }
      shift = on;
    }
  }
  __syncthreads();
  const bool sh = shift != 0;
  const float mu = sh ? stat[0] : 0.f, sig = sh ? stat[1] : 1.f;
  const long long total = (long long)B * T;
  for (long long i = blockIdx.x * (long long)SYN_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * SYN_BLOCK) {
    const int b = (int)(i / T), t = (int)(i - (long long)b * T);
    const bool valid = t < lens[b];
    const bool v = valid && voiced_of(vl[b * vs + t]);
    float f = 0.f;
    if (v) {
      f = f0[b * f0s + t];
      if (sh) f = __fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(f, mu), sig), f0_std[b]), f0_mean[b]);
    }
    f0o[i] = f;
    vo[i] = v ? 1.f : 0.f;
    eno[i] = valid ? en[b * ens + t] : 0.f;
  }
}

inline int grid_for(long long total) {
  long long g = (total + SYN_BLOCK - 1) / SYN_BLOCK;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int radmmm_synth_durations(const float* x, int64_t item_stride, const int32_t* text_lens, int B, int Tt,
                                      int integer_mode, int32_t* dur, int32_t* cum, int32_t* out_lens,
                                      radmmm_stream_t stream) {
  RADMMM_REQUIRE(x && dur && cum && out_lens, "synth_durations: null pointer");
  RADMMM_REQUIRE(B > 0 && Tt > 0 && Tt <= SYN_MAX_TT && item_stride >= Tt,
                 "synth_durations: bad dims (B=%d Tt=%d item_stride=%lld)", B, Tt, (long long)item_stride);
  hipLaunchKernelGGL(durations_kernel, dim3(B), dim3(SYN_BLOCK), 0, ST(stream), x, (long long)item_stride, Tt, text_lens,
                     integer_mode ? 1 : 0, dur, cum, out_lens);
  return radmmm::check_launch("synth_durations");
}

extern "C" int radmmm_synth_regulate(const float* txt, int64_t item_stride, int row_stride, int Tt, int C,
                                     const int32_t* cum, const int32_t* out_lens, int B, int Tmax, float* rows, int ldc,
                                     radmmm_stream_t stream) {
  RADMMM_REQUIRE(txt && cum && out_lens && rows, "synth_regulate: null pointer");
  RADMMM_REQUIRE(B > 0 && Tt > 0 && Tt <= REG_MAX_TT && C > 0 && C % 4 == 0 && ldc % 4 == 0 && ldc >= C && Tmax > 0 &&
                     row_stride >= C && row_stride % 4 == 0 && item_stride >= (int64_t)(Tt - 1) * row_stride + C &&
                     item_stride % 4 == 0,
                 "synth_regulate: bad dims (B=%d Tt=%d C=%d ldc=%d Tmax=%d row_stride=%d item_stride=%lld)", B, Tt, C,
                 ldc, Tmax, row_stride, (long long)item_stride);
  RADMMM_REQUIRE(radmmm::aligned16(txt) && radmmm::aligned16(rows), "synth_regulate: txt / rows must be 16B aligned");
  const dim3 grid((Tmax + REG_FRAMES - 1) / REG_FRAMES, B);
  hipLaunchKernelGGL(regulate_kernel, grid, dim3(SYN_BLOCK), (Tt + REG_FRAMES) * sizeof(int), ST(stream), txt,
                     (long long)item_stride, row_stride, Tt, C, cum, out_lens, rows, ldc, Tmax);
  return radmmm::check_launch("synth_regulate");
}

extern "C" int radmmm_synth_f0_stats(const float* f0, int64_t f0_stride, const float* voiced_logit, int64_t v_stride,
                                     const int32_t* lens, int B, int T, double* partials, int nparts,
                                     radmmm_stream_t stream) {
  RADMMM_REQUIRE(f0 && voiced_logit && lens && partials, "synth_f0_stats: null pointer");
  RADMMM_REQUIRE(B > 0 && T > 0 && f0_stride >= T && v_stride >= T && nparts >= 1 && nparts <= F0_MAX_PARTS,
                 "synth_f0_stats: bad dims (B=%d T=%d nparts=%d)", B, T, nparts);
  hipLaunchKernelGGL(f0_stats_kernel, dim3(nparts), dim3(SYN_BLOCK), 0, ST(stream), f0, (long long)f0_stride,
                     voiced_logit, (long long)v_stride, lens, B, T, partials, nparts);
  return radmmm::check_launch("synth_f0_stats");
}

extern "C" int radmmm_synth_f0_apply(const float* f0, int64_t f0_stride, const float* voiced_logit, int64_t v_stride,
                                     const float* energy, int64_t e_stride, const int32_t* lens, int B, int T,
                                     const double* partials, int nparts, const float* f0_mean, const float* f0_std,
                                     float* f0_out, float* energy_out, float* voiced_out, radmmm_stream_t stream) {
  RADMMM_REQUIRE(f0 && voiced_logit && energy && lens && f0_out && energy_out && voiced_out,
                 "synth_f0_apply: null pointer");
  RADMMM_REQUIRE(!partials || (f0_mean && f0_std), "synth_f0_apply: shift stats need f0_mean and f0_std");
  RADMMM_REQUIRE(B > 0 && T > 0 && f0_stride >= T && v_stride >= T && e_stride >= T &&
                     (!partials || (nparts >= 1 && nparts <= F0_MAX_PARTS)),
                 "synth_f0_apply: bad dims (B=%d T=%d nparts=%d)", B, T, nparts);
  hipLaunchKernelGGL(f0_apply_kernel, dim3(grid_for((long long)B * T)), dim3(SYN_BLOCK), 0, ST(stream), f0,
                     (long long)f0_stride, voiced_logit, (long long)v_stride, energy, (long long)e_stride, lens, B, T,
                     partials, nparts, f0_mean, f0_std, f0_out, energy_out, voiced_out);
  return radmmm::check_launch("synth_f0_apply");
}
