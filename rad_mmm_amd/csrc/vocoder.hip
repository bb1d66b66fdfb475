// HiFi-GAN generator and STFT denoiser support kernels (vocoders/hifigan_models.py:104-247,
// vocoders/hifigan_denoiser.py:25-58, audio_processing.py:195-291) on gfx950.
//
// The convolutions themselves (conv_pre, every resblock conv, the polyphase transposed convs
// and the inverse STFT's overlap-add) are row GEMMs of radmmm_rowgemm_f32; what lives here is
// everything around them, in the same channels-last row layout ([B*T rows][ld] fp32, row
// r = b*T + t) and with the same per-item length masking (rows at or past an item's length are
// zeros on load and are written as zeros):
//   radmmm_voc_lrelu        the operand of every conv: leaky_relu(x / div), masked
//   radmmm_voc_conv_post    conv_post (C -> 1, k taps) + tanh as a per-row reduction
//   radmmm_voc_reflect_pad  the STFT's reflect pad at each item's own length
//   radmmm_voc_spec_bins    the denoiser's magnitude clamp as a rescale of each complex bin
//   radmmm_voc_istft_finish the window-sum division, hop scale and trim of the inverse STFT
//   radmmm_voc_normalize    audio / max|audio| over each item's valid samples
#include <float.h>

#include "common.h"

namespace {

using radmmm::grid_for;
using radmmm::lrelu;
using radmmm::ST;

// y[r, c] = lrelu(x[r, c] / div) for t < lens[b] (c < cols), 0 otherwise and in the padding columns
// cols <= c < ldy.  ldx, ldy % 4 == 0: one float4 per thread.  x and y carry no __restrict__: the generator calls this
// in place (y == x, ldy == ldx), where every thread loads its float4 before it stores the same four floats.
__global__ __launch_bounds__(256) void lrelu_kernel(const float* x, int ldx, float* y, int ldy, long long rows, int cols,
                                                    int T, const int32_t* __restrict__ lens, float div, float slope) {
  const int q = ldy >> 2;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 4;
    const int b = (int)(r / T), t = (int)(r - (long long)b * T);
    const bool valid = !lens || t < lens[b];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid && c < cols) {
      const float4 v = *reinterpret_cast<const float4*>(x + r * ldx + c);
      o.x = lrelu(v.x / div, slope);
      o.y = c + 1 < cols ? lrelu(v.y / div, slope) : 0.f;
      o.z = c + 2 < cols ? lrelu(v.z / div, slope) : 0.f;
      o.w = c + 3 < cols ? lrelu(v.w / div, slope) : 0.f;
    }
    *reinterpret_cast<float4*>(y + r * ldy + c) = o;
  }
}

// out[r] = tanh(bias + sum_tap sum_c lrelu(x[r + tap - taps/2, c] / div) * w[tap * ldw + c]) for t < lens[b], else 0.
// One row per thread; the weights (taps x C <= 4096 floats) sit in LDS.
constexpr int POST_MAX_W = 4096;
__global__ __launch_bounds__(256) void conv_post_kernel(const float* __restrict__ x, int ldx,
                                                        const float* __restrict__ w, int ldw,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        long long rows, int C, int taps, int T,
                                                        const int32_t* __restrict__ lens, float div, float slope) {
  __shared__ float ws[POST_MAX_W];
  for (int i = threadIdx.x; i < taps * ldw; i += blockDim.x) ws[i] = w[i];
  __syncthreads();
  const float b0 = bias ? bias[0] : 0.f;
  for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < rows;
       r += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(r / T), t = (int)(r - (long long)b * T);
    const int len = lens ? lens[b] : T;
    float v = 0.f;
    if (t < len) {
      float acc = 0.f;
      for (int tap = 0; tap < taps; ++tap) {
        const int ts = t + tap - taps / 2;
        if (ts < 0 || ts >= len) continue;
        const float* xr = x + (r + (ts - t)) * ldx;
        const float* wr = ws + tap * ldw;
        for (int c = 0; c < C; c += 4) {
          const float4 xv = *reinterpret_cast<const float4*>(xr + c);
          acc = fmaf(lrelu(xv.x / div, slope), wr[c], acc);
          if (c + 1 < C) acc = fmaf(lrelu(xv.y / div, slope), wr[c + 1], acc);
          if (c + 2 < C) acc = fmaf(lrelu(xv.z / div, slope), wr[c + 2], acc);
          if (c + 3 < C) acc = fmaf(lrelu(xv.w / div, slope), wr[c + 3], acc);
        }
      }
      v = tanhf(acc + b0);
    }
    out[r] = v;
  }
}

// xpad[b*pitch + p] = audio[b*lda + reflect(p - pad)] for p < lens[b] + 2 pad (reflect without edge repeat inside
// [0, lens[b])), 0 beyond.  lens[b] > pad is the caller's precondition (the reference's F.pad(mode='reflect') raises
// otherwise); the index is clamped so that a violation cannot read outside the item.
__global__ __launch_bounds__(256) void reflect_pad_kernel(const float* __restrict__ audio, int lda,
                                                          const int32_t* __restrict__ lens, float* __restrict__ xpad,
                                                          int B, int S, int pad, int pitch) {
  const long long total = (long long)B * pitch;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / pitch), p = (int)(i - (long long)b * pitch);
    int len = lens ? lens[b] : S;
    len = len < S ? len : S;
    float v = 0.f;
    if (len > 0 && p < len + 2 * pad) {
      int j = p - pad;
      if (j < 0) j = -j;
      if (j >= len) j = 2 * (len - 1) - j;
      j = j < 0 ? 0 : (j >= len ? len - 1 : j);
      v = audio[(long long)b * lda + j];
    }
    xpad[i] = v;
  }
}

// spec row r: re at columns [0, cutoff), im at [cutoff, 2 cutoff).  mag = |re + i im|,
// mag' = max(mag - bias[c] * strength, 0); (re, im) <- (re, im) * mag' / mag, or (mag', 0) where mag == 0
// (atan2(0, 0) = 0 in the reference's magnitude / phase round trip).  mag_out != NULL: write mag[r * cutoff + c]
// instead and leave spec alone (the denoiser's bias spectrum).
__global__ __launch_bounds__(256) void spec_bins_kernel(float* __restrict__ spec, int lds, long long rows, int cutoff,
                                                        const float* __restrict__ bias, float strength,
                                                        float* __restrict__ mag_out) {
  const long long total = rows * cutoff;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / cutoff;
    const int c = (int)(i - r * cutoff);
    float* row = spec + r * lds;
    const float re = row[c], im = row[cutoff + c];
    const float mag = sqrtf(re * re + im * im);
    if (mag_out) {
      mag_out[i] = mag;
      continue;
    }
    const float m2 = fmaxf(mag - bias[c] * strength, 0.f);
    if (mag > 0.f) {
      const float s = m2 / mag;
      row[c] = re * s;
      row[cutoff + c] = im * s;
    } else {
      row[c] = m2;
      row[cutoff + c] = 0.f;
    }
  }
}

// y [B][pitch] holds the overlap-add of the inverse basis already shifted by n_fft/2 samples (the trim).  Sample n of
// item b (n < (frames[b] - 1) * hop) is divided by the window sum-square envelope of frames[b] frames at position
// m = n + n_fft/2 where that exceeds FLT_MIN, then scaled by n_fft / hop; samples past the item's length become 0.
// The envelope is accumulated as the reference's window_sumsquare does: fp32 running sum, fp64 terms, frame order.
__global__ __launch_bounds__(256) void istft_finish_kernel(float* __restrict__ y, int B, int pitch,
                                                           const int32_t* __restrict__ frames,
                                                           const double* __restrict__ winsq, int n_fft, int hop,
                                                           float scale) {
  const long long total = (long long)B * pitch;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / pitch), n = (int)(i - (long long)b * pitch);
    const int nf = frames[b];
    if (n >= (nf - 1) * hop) {
      y[i] = 0.f;
      continue;
    }
    const int m = n + n_fft / 2;
    int f0 = m - n_fft + 1;
    f0 = f0 <= 0 ? 0 : (f0 + hop - 1) / hop;
    int f1 = m / hop;
    if (f1 > nf - 1) f1 = nf - 1;
    float ws = 0.f;
    for (int f = f0; f <= f1; ++f) ws = (float)((double)ws + winsq[m - f * hop]);
    float v = y[i];
    if (ws > FLT_MIN) v = v / ws;
    y[i] = v * scale;
  }
}

// audio[b, :lens[b]] /= max|audio[b, :lens[b]]| (a division, like the reference); samples at or past lens[b] are
// neither read nor written.  An all-zero item becomes NaN (0 / 0), as the reference's audio / max|audio| does.  One
// workgroup per item.
__global__ __launch_bounds__(1024) void normalize_kernel(float* __restrict__ audio, int lda,
                                                         const int32_t* __restrict__ lens, int S) {
  __shared__ float sh[17];
  const int b = blockIdx.x;
  float* a = audio + (long long)b * lda;
  int len = lens ? lens[b] : S;
  len = len < S ? len : S;
  float m = 0.f;
  for (int i = threadIdx.x; i < len; i += blockDim.x) m = fmaxf(m, fabsf(a[i]));
  m = radmmm::wave_max(m);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) sh[w] = m;
  __syncthreads();
  if (w == 0) {
    float t = lane < nw ? sh[lane] : 0.f;
    t = radmmm::wave_max(t);
    if (lane == 0) sh[16] = t;
  }
  __syncthreads();
  const float mx = sh[16];
  for (int i = threadIdx.x; i < len; i += blockDim.x) a[i] = a[i] / mx;
}

}  // namespace

extern "C" int radmmm_voc_lrelu(const float* x, int ldx, float* y, int ldy, int rows, int cols, int T,
                                const int32_t* lens, float div, float slope, radmmm_stream_t stream) {
  RADMMM_REQUIRE(x && y, "voc_lrelu: null pointer");
  RADMMM_REQUIRE(rows > 0 && cols > 0 && T > 0 && rows % T == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= cols &&
                     ldy >= cols && div != 0.f,
                 "voc_lrelu: bad dims (rows=%d cols=%d T=%d ldx=%d ldy=%d)", rows, cols, T, ldx, ldy);
  RADMMM_REQUIRE(radmmm::aligned16(x) && radmmm::aligned16(y), "voc_lrelu: x / y must be 16B aligned");
  const long long total = (long long)rows * (ldy / 4);
  hipLaunchKernelGGL(lrelu_kernel, dim3(grid_for(total, 256)), dim3(256), 0, ST(stream), x, ldx, y, ldy,
                     (long long)rows, cols, T, lens, div, slope);
  return radmmm::check_launch("voc_lrelu");
}

extern "C" int radmmm_voc_conv_post(const float* x, int ldx, const float* w, int ldw, const float* bias, float* out,
                                    int rows, int C, int taps, int T, const int32_t* lens, float div, float slope,
                                    radmmm_stream_t stream) {
  RADMMM_REQUIRE(x && w && out, "voc_conv_post: null pointer");
  RADMMM_REQUIRE(rows > 0 && C > 0 && taps >= 1 && taps % 2 == 1 && T > 0 && rows % T == 0 && ldx % 4 == 0 &&
                     ldx >= ((C + 3) & ~3) && ldw >= C && taps * ldw <= POST_MAX_W && div != 0.f,
                 "voc_conv_post: bad dims (rows=%d C=%d taps=%d T=%d ldx=%d ldw=%d)", rows, C, taps, T, ldx, ldw);
  RADMMM_REQUIRE(radmmm::aligned16(x), "voc_conv_post: x must be 16B aligned");
  hipLaunchKernelGGL(conv_post_kernel, dim3(grid_for(rows, 256)), dim3(256), 0, ST(stream), x, ldx, w, ldw, bias, out,
                     (long long)rows, C, taps, T, lens, div, slope);
  return radmmm::check_launch("voc_conv_post");
}

extern "C" int radmmm_voc_reflect_pad(const float* audio, int lda, const int32_t* lens, float* xpad, int B, int S,
                                      int pad, int pitch, radmmm_stream_t stream) {
  RADMMM_REQUIRE(audio && xpad, "voc_reflect_pad: null pointer");
  RADMMM_REQUIRE(B > 0 && S > pad && pad >= 0 && lda >= S && pitch >= S + 2 * pad,
                 "voc_reflect_pad: bad dims (B=%d S=%d pad=%d pitch=%d)", B, S, pad, pitch);
  hipLaunchKernelGGL(reflect_pad_kernel, dim3(grid_for((long long)B * pitch, 256)), dim3(256), 0, ST(stream), audio,
                     lda, lens, xpad, B, S, pad, pitch);
  return radmmm::check_launch("voc_reflect_pad");
}

extern "C" int radmmm_voc_spec_bins(float* spec, int lds, int rows, int cutoff, const float* bias, float strength,
                                    float* mag_out, radmmm_stream_t stream) {
  RADMMM_REQUIRE(spec && (bias || mag_out), "voc_spec_bins: null pointer");
  RADMMM_REQUIRE(rows > 0 && cutoff > 0 && lds >= 2 * cutoff, "voc_spec_bins: bad dims (rows=%d cutoff=%d lds=%d)", rows,
                 cutoff, lds);
  hipLaunchKernelGGL(spec_bins_kernel, dim3(grid_for((long long)rows * cutoff, 256)), dim3(256), 0, ST(stream), spec,
                     lds, (long long)rows, cutoff, bias, strength, mag_out);
  return radmmm::check_launch("voc_spec_bins");
}

extern "C" int radmmm_voc_istft_finish(float* y, int B, int pitch, const int32_t* frames, const double* winsq, int n_fft,
                                       int hop, radmmm_stream_t stream) {
  RADMMM_REQUIRE(y && frames && winsq, "voc_istft_finish: null pointer");
  RADMMM_REQUIRE(B > 0 && pitch > 0 && n_fft > 0 && hop > 0 && n_fft % hop == 0 && n_fft % 2 == 0,
                 "voc_istft_finish: bad dims (B=%d pitch=%d n_fft=%d hop=%d)", B, pitch, n_fft, hop);
  hipLaunchKernelGGL(istft_finish_kernel, dim3(grid_for((long long)B * pitch, 256)), dim3(256), 0, ST(stream), y, B,
                     pitch, frames, winsq, n_fft, hop, (float)n_fft / (float)hop);
  return radmmm::check_launch("voc_istft_finish");
}

extern "C" int radmmm_voc_normalize(float* audio, int lda, const int32_t* lens, int B, int S, radmmm_stream_t stream) {
  RADMMM_REQUIRE(audio, "voc_normalize: null pointer");
  RADMMM_REQUIRE(B > 0 && S > 0 && lda >= S, "voc_normalize: bad dims (B=%d S=%d lda=%d)", B, S, lda);
  hipLaunchKernelGGL(normalize_kernel, dim3(B), dim3(1024), 0, ST(stream), audio, lda, lens, S);
  return radmmm::check_launch("voc_normalize");
}
