// WaveGlow inference support kernels (vocoders/waveglow_for_LIMMITS23/glow.py:105-175 WN.forward, :251-293
// WaveGlow.infer) on gfx950.
//
// The wide convolutions (the polyphase upsample, cond_layer, the dilated in_layers and the 1x1 res_skip layers) are
// row GEMMs of radmmm_rowgemm_f32; what lives here is everything around them, on channels-last rows of GROUP steps
// ([B*Tg rows][ld] fp32, row r = b*Tg + g, Tg = T*hop/n_group) with the same per-item length masking as the HiFi-GAN
// path (rows at or past lens[b] are written as zeros, so no layer ever sees what bias and gating would leave there):
//   radmmm_wg_group_cond    upsampled mel [B][Tg*n_group][n_mel] -> conditioning rows [B*Tg][n_mel*n_group]
//   radmmm_wg_noise_rows    sigma * z (reference layout [B][ch][Tg]) into `ch` columns of the audio rows: the initial
//                           draw and every early re-attachment (the audio rows are kept RIGHT aligned in n_group
//                           columns, so cat(sigma*z, audio) is a write beside the live columns and nothing moves)
//   radmmm_wg_start         WN.start: n_half (<= 8) -> C channels, K far below a GEMM tile
//   radmmm_wg_gate          tanh(a[:, :C] + cond[:, off:off+C]) * sigmoid(a[:, C:] + cond[:, off+C:off+2C])
//   radmmm_wg_res_skip      audio += rs[:, :C]; skip (+)= rs[:, C:]   (last layer: skip += rs[:, :C] only)
//   radmmm_wg_start_split / wg_gate_split / wg_res_skip_split   the three above for the 16-bit GEMM modes: they also
//                           write the next GEMM's split f16 operand (hi, lo) in the same pass
//   radmmm_wg_end_coupling  WN.end (C -> 2 n_half) + audio_1 = (audio_1 - b) * exp(-s) + the inverse 1x1 mix, in place
//   radmmm_wg_ungroup       audio rows -> [B][Tg*n_group] samples, zeros past each length
// and the other direction (glow.py:207-249 WaveGlow.forward: audio -> latent, with the terms of its likelihood), which
// runs the same WN launches on the untouched half:
//   radmmm_wg_group_audio       [B][Tg*n_group] samples -> audio rows (the inverse of wg_ungroup)
//   radmmm_wg_mix_fwd           the forward 1x1 mix W on the live columns, in place
//   radmmm_wg_end_coupling_fwd  WN.end + audio_1 = exp(log_s) * audio_1 + b, in place, + the row's sum of log_s
//   radmmm_wg_nll_parts         per item: sum of z^2 and sum of the rows' log_s sums over its valid rows, in float64
// All of them are bound by memory traffic (each reads or writes [rows][C] or [rows][2C] once); none uses atomics and
// every output element is summed in an order that depends on its own row alone, so an item in a batch is bit-identical
// to the item alone as far as these kernels go (wg_nll_parts: on the item's own rows alone, in a fixed order).
#include "common.h"
#include "split_pack.h"

namespace {

using radmmm::ST;

inline int grid_for(long long total, int block) {
  long long g = (total + block - 1) / block;
  if (g > 16384) g = 16384;
  if (g < 1) g = 1;
  return (int)g;
}

// rows[(b*Tg + g)*ldr + m*ng + j] = up[b*item_stride + (g*ng + j)*n_mel + m] for g < lens[b]; 0 in the rows past the
// item's length and in the padding columns n_mel*ng <= c < ldr.  One thread per output element: a group step's source
// (ng x n_mel floats) and destination (n_mel x ng) are the same contiguous 4*n_mel*ng bytes transposed, so both sides
// stay inside a few cache lines per wavefront.
__global__ __launch_bounds__(256) void group_cond_kernel(const float* __restrict__ up, long long item_stride,
                                                         float* __restrict__ rows, int ldr,
                                                         const int32_t* __restrict__ lens, long long R, int Tg,
                                                         int n_mel, int ng) {
  const long long total = R * ldr;
  const int cols = n_mel * ng;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / ldr;
    const int c = (int)(i - r * ldr);
    const int b = (int)(r / Tg), g = (int)(r - (long long)b * Tg);
    float v = 0.f;
    if (c < cols && (!lens || g < lens[b])) {
      const int m = c / ng, j = c - m * ng;
      v = up[b * item_stride + ((long long)g * ng + j) * n_mel + m];
    }
    rows[i] = v;
  }
}

// X[(b*Tg + g)*ldx + col0 + c] = sigma * z[(b*ch + c)*Tg + g] for g < lens[b], else 0
__global__ __launch_bounds__(256) void noise_rows_kernel(const float* __restrict__ z, float sigma,
                                                         float* __restrict__ X, int ldx, int col0, int ch,
                                                         const int32_t* __restrict__ lens, int B, int Tg) {
  const long long total = (long long)B * ch * Tg;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long bc = i / Tg;
    const int g = (int)(i - bc * Tg);
    const int b = (int)(bc / ch), c = (int)(bc - (long long)b * ch);
    const bool valid = !lens || g < lens[b];
    X[((long long)b * Tg + g) * ldx + col0 + c] = valid ? sigma * z[i] : 0.f;
  }
}

// H[r, c] = bias[c] + sum_{i < nh} W[c*nh + i] * X[r*ldx + col0 + i] for t < lens[b], else 0.  One float4 of H per
// thread; the nh <= 8 inputs of the row are re-read by the C/4 threads of the row (L1 hits).
constexpr int START_MAX_NH = 8;
__global__ __launch_bounds__(256) void start_kernel(const float* __restrict__ X, int ldx, int col0, int nh,
                                                    const float* __restrict__ W, const float* __restrict__ bias,
                                                    float* __restrict__ H, int ldh, int C,
                                                    const int32_t* __restrict__ lens, long long rows, int T) {
  const int q = C >> 2;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 4;
    const int b = (int)(r / T), t = (int)(r - (long long)b * T);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (!lens || t < lens[b]) {
      const float* xr = X + r * ldx + col0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float acc = bias ? bias[c + e] : 0.f;
        const float* w = W + (long long)(c + e) * nh;
        for (int k = 0; k < nh; ++k) acc = fmaf(w[k], xr[k], acc);
        o[e] = acc;
      }
    }
    *reinterpret_cast<float4*>(H + r * ldh + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

__device__ __forceinline__ float gate1(float ta, float tc, float sa, float sc) {
  // libm tanhf / expf (not the 1-ulp hardware exp2 forms): the kernel is bound by its 5 C floats of traffic per row
  return tanhf(ta + tc) * (1.f / (1.f + expf(-(sa + sc))));
}

// y[r, c] = tanh(a[r, c] + cond[r, off + c]) * sigmoid(a[r, C + c] + cond[r, off + C + c]) for t < lens[b], else 0
__global__ __launch_bounds__(256) void gate_kernel(const float* __restrict__ a, int lda, const float* __restrict__ cond,
                                                   int ldcond, int off, float* __restrict__ y, int ldy, int C,
                                                   const int32_t* __restrict__ lens, long long rows, int T) {
  const int q = C >> 2;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 4;
    const int b = (int)(r / T), t = (int)(r - (long long)b * T);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!lens || t < lens[b]) {
      const float* ar = a + r * lda + c;
      const float* cr = cond + r * ldcond + off + c;
      const float4 ta = *reinterpret_cast<const float4*>(ar), sa = *reinterpret_cast<const float4*>(ar + C);
      const float4 tc = *reinterpret_cast<const float4*>(cr), sc = *reinterpret_cast<const float4*>(cr + C);
      o.x = gate1(ta.x, tc.x, sa.x, sc.x);
      o.y = gate1(ta.y, tc.y, sa.y, sc.y);
      o.z = gate1(ta.z, tc.z, sa.z, sc.z);
      o.w = gate1(ta.w, tc.w, sa.w, sc.w);
    }
    *reinterpret_cast<float4*>(y + r * ldy + c) = o;
  }
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// not last: H[r, c] += rs[r, c]; S[r, c] = (first ? 0 : S[r, c]) + rs[r, C + c].  last: S[r, c] = (first ? 0 : S[r, c])
// + rs[r, c], H untouched.  Rows past the item's length are written as zeros in everything that is written.
__global__ __launch_bounds__(256) void res_skip_kernel(const float* __restrict__ rs, int ldrs, float* __restrict__ H,
                                                       int ldh, float* __restrict__ S, int lds, int C, int first,
                                                       int last, const int32_t* __restrict__ lens, long long rows,
                                                       int T) {
  const int q = C >> 2;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 4;
    const int b = (int)(r / T), t = (int)(r - (long long)b * T);
    const bool valid = !lens || t < lens[b];
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f), s = h;
    float4* hp = last ? nullptr : reinterpret_cast<float4*>(H + r * ldh + c);   // H may be NULL with last
    float4* sp = reinterpret_cast<float4*>(S + r * lds + c);
    if (valid) {
      const float* rr = rs + r * ldrs + c;
      if (!first) s = *sp;
      if (last) {
        s = add4(s, *reinterpret_cast<const float4*>(rr));
      } else {
        h = add4(*hp, *reinterpret_cast<const float4*>(rr));
        s = add4(s, *reinterpret_cast<const float4*>(rr + C));
      }
    }
    if (!last) *hp = h;
    *sp = s;
  }
}

// ---- the same three kernels for the 16-bit GEMM modes ("h3" / "f16" of WaveGlow.infer) --------------------------------
// Each writes the split operand of the GEMM that follows (split_pack.h: hi = fp16(x), lo = fp16(x - hi), scale 1; the
// bits of radmmm_split_f16 of the fp32 value) in the pass that computes the value, instead of a pass of its own over
// [rows][C].  A thread owns 8 columns of a row: two float4 per fp32 array, one 16-byte store per half array.  The pair
// arrays are [rows][ldp] halves; the padding columns C <= c < ldp and the rows at or past an item's length are written
// as zeros in both halves, and nothing is read there (a select, as in the twins above).  Pl == NULL: the lo half is not
// written (single-product mode).  The fp32 arithmetic is the twin's, operation for operation: the same bits.

__device__ __forceinline__ void zero8(float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.f;
}

__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// start_kernel + the pair of H
__global__ __launch_bounds__(256) void start_split_kernel(const float* __restrict__ X, int ldx, int col0, int nh,
                                                          const float* __restrict__ W, const float* __restrict__ bias,
                                                          float* __restrict__ H, int ldh, void* __restrict__ Ph,
                                                          void* __restrict__ Pl, int ldp, int C,
                                                          const int32_t* __restrict__ lens, long long rows, int T) {
  const int q = ldp >> 3;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 8;
    float o[8];
    zero8(o);
    if (c < C) {
      const int b = (int)(r / T), t = (int)(r - (long long)b * T);
      if (!lens || t < lens[b]) {
        const float* xr = X + r * ldx + col0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float acc = bias ? bias[c + e] : 0.f;
          const float* w = W + (long long)(c + e) * nh;
          for (int k = 0; k < nh; ++k) acc = fmaf(w[k], xr[k], acc);
          o[e] = acc;
        }
      }
      store8(H + r * ldh + c, o);
    }
    radmmm::store_split8_f16(Ph, Pl, r * ldp, c, 1.f, o);
  }
}

// gate_kernel, its result as a pair only
__global__ __launch_bounds__(256) void gate_split_kernel(const float* __restrict__ a, int lda,
                                                         const float* __restrict__ cond, int ldcond, int off,
                                                         void* __restrict__ Ph, void* __restrict__ Pl, int ldp, int C,
                                                         const int32_t* __restrict__ lens, long long rows, int T) {
  const int q = ldp >> 3;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 8;
    float o[8];
    zero8(o);
    if (c < C) {
      const int b = (int)(r / T), t = (int)(r - (long long)b * T);
      if (!lens || t < lens[b]) {
        float ta[8], sa[8], tc[8], sc[8];
        const float* ar = a + r * lda + c;
        const float* cr = cond + r * ldcond + off + c;
        load8(ar, ta);
        load8(ar + C, sa);
        load8(cr, tc);
        load8(cr + C, sc);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = gate1(ta[e], tc[e], sa[e], sc[e]);
      }
    }
    radmmm::store_split8_f16(Ph, Pl, r * ldp, c, 1.f, o);
  }
}

// res_skip_kernel + the pair of the updated H (not last; with last nothing but S is written)
__global__ __launch_bounds__(256) void res_skip_split_kernel(const float* __restrict__ rs, int ldrs,
                                                             float* __restrict__ H, int ldh, float* __restrict__ S,
                                                             int lds, void* __restrict__ Ph, void* __restrict__ Pl,
                                                             int ldp, int C, int first, int last,
                                                             const int32_t* __restrict__ lens, long long rows, int T) {
  const int q = (last ? C : ldp) >> 3;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 8;
    float h[8], s[8];
    zero8(h);
    zero8(s);
    if (c < C) {
      const int b = (int)(r / T), t = (int)(r - (long long)b * T);
      float* sp = S + r * lds + c;
      if (!lens || t < lens[b]) {
        const float* rr = rs + r * ldrs + c;
        float x[8];
        if (!first) load8(sp, s);
        if (last) {
          load8(rr, x);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] = s[e] + x[e];
        } else {
          load8(H + r * ldh + c, h);
          load8(rr, x);
#pragma unroll
          for (int e = 0; e < 8; ++e) h[e] = h[e] + x[e];
          load8(rr + C, x);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] = s[e] + x[e];
        }
      }
      if (!last) store8(H + r * ldh + c, h);
      store8(sp, s);
    }
    if (!last) radmmm::store_split8_f16(Ph, Pl, r * ldp, c, 1.f, h);
  }
}

// The part the two coupling kernels share: o = Wend S[r] (NO = 2 n_half outputs, bend is added by the caller).  16 lanes
// share a row (a float4 of S per lane and 64 columns, xor-butterfly over the 16 lanes: every row is summed in the same
// order wherever it sits), 16 rows per workgroup pass, Wend [NO][C] in LDS at w.
template <int NO>
__device__ __forceinline__ void end_dot(const float* __restrict__ S, int lds, const float* w, int C, long long r,
                                        bool valid, int sub, float (&acc)[NO]) {
#pragma unroll
  for (int o = 0; o < NO; ++o) acc[o] = 0.f;
  if (valid) {
    const float* sr = S + r * lds;
    for (int c = sub * 4; c < C; c += 64) {
      const float4 v = *reinterpret_cast<const float4*>(sr + c);
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const float4 ww = *reinterpret_cast<const float4*>(w + o * C + c);
        acc[o] = fmaf(v.w, ww.w, fmaf(v.z, ww.z, fmaf(v.y, ww.y, fmaf(v.x, ww.x, acc[o]))));
      }
    }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) {
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) acc[o] += __shfl_xor(acc[o], m, 16);
  }
}

__device__ __forceinline__ bool row_valid(long long r, long long rows, const int32_t* lens, int T) {
  if (r >= rows) return false;
  if (!lens) return true;
  const int b = (int)(r / T), t = (int)(r - (long long)b * T);
  return t < lens[b];
}

// out = Wend S[r] + bend (NO = 2 n_half outputs: b = out[:n_half], s = out[n_half:]), z = [X0, (X1 - b) * exp(-s)],
// X[r, col0 : col0 + NO] = Winv z; zeros past the item's length.  Wend / Winv / bend in LDS, the sum as end_dot.
template <int NO>
__global__ __launch_bounds__(256) void end_coupling_kernel(const float* __restrict__ S, int lds,
                                                           const float* __restrict__ Wend,
                                                           const float* __restrict__ bend,
                                                           const float* __restrict__ Winv, float* __restrict__ X,
                                                           int ldx, int col0, int C,
                                                           const int32_t* __restrict__ lens, long long rows, int T) {
  extern __shared__ __align__(16) float sh[];   // float4 reads of Wend rows in end_dot
  float* w = sh;                    // [NO][C]
  float* wi = sh + NO * C;          // [NO][NO]
  float* be = wi + NO * NO;         // [NO]
  for (int i = threadIdx.x; i < NO * C; i += blockDim.x) w[i] = Wend[i];
  for (int i = threadIdx.x; i < NO * NO; i += blockDim.x) wi[i] = Winv[i];
  for (int i = threadIdx.x; i < NO; i += blockDim.x) be[i] = bend ? bend[i] : 0.f;
  __syncthreads();
  constexpr int NH = NO / 2;
  const int sub = threadIdx.x & 15, rloc = threadIdx.x >> 4;
  for (long long r0 = blockIdx.x * 16LL; r0 < rows; r0 += gridDim.x * 16LL) {
    const long long r = r0 + rloc;
    const bool valid = row_valid(r, rows, lens, T);
    float acc[NO];
    end_dot<NO>(S, lds, w, C, r, valid, sub, acc);
    if (sub == 0 && r < rows) {
      float* xr = X + r * ldx + col0;
      float z[NO];
      if (valid) {
#pragma unroll
        for (int k = 0; k < NH; ++k) {
          z[k] = xr[k];
          z[NH + k] = (xr[NH + k] - (acc[k] + be[k])) * expf(-(acc[NH + k] + be[NH + k]));
        }
#pragma unroll
        for (int o = 0; o < NO; ++o) {
          float v = 0.f;
#pragma unroll
          for (int k = 0; k < NO; ++k) v = fmaf(wi[o * NO + k], z[k], v);
          xr[o] = v;
        }
      } else {
#pragma unroll
        for (int o = 0; o < NO; ++o) xr[o] = 0.f;
      }
    }
  }
}

// The forward counterpart: o = Wend S[r] + bend, b = o[:n_half], log_s = o[n_half:]; X1 = exp(log_s) * X1 + b in place
// (X0 is not touched), ls[r] = (first ? 0 : ls[r]) + sum_i log_s[i], and with logs != NULL logs[r*n_half + i] =
// log_s[i].  Rows past the item's length: X1, ls[r] and logs are written as 0.
template <int NO>
__global__ __launch_bounds__(256) void end_coupling_fwd_kernel(const float* __restrict__ S, int lds,
                                                               const float* __restrict__ Wend,
                                                               const float* __restrict__ bend, float* __restrict__ X,
                                                               int ldx, int col0, int C, float* __restrict__ ls,
                                                               int first, float* __restrict__ logs,
                                                               const int32_t* __restrict__ lens, long long rows,
                                                               int T) {
  extern __shared__ __align__(16) float sh[];
  float* w = sh;                    // [NO][C]
  float* be = sh + NO * C;          // [NO]
  for (int i = threadIdx.x; i < NO * C; i += blockDim.x) w[i] = Wend[i];
  for (int i = threadIdx.x; i < NO; i += blockDim.x) be[i] = bend ? bend[i] : 0.f;
  __syncthreads();
  constexpr int NH = NO / 2;
  const int sub = threadIdx.x & 15, rloc = threadIdx.x >> 4;
  for (long long r0 = blockIdx.x * 16LL; r0 < rows; r0 += gridDim.x * 16LL) {
    const long long r = r0 + rloc;
    const bool valid = row_valid(r, rows, lens, T);
    float acc[NO];
    end_dot<NO>(S, lds, w, C, r, valid, sub, acc);
    if (sub == 0 && r < rows) {
      float* x1 = X + r * ldx + col0 + NH;
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        float v = 0.f, l = 0.f;
        if (valid) {
          l = acc[NH + k] + be[NH + k];
          v = fmaf(expf(l), x1[k], acc[k] + be[k]);
          sum += l;
        }
        x1[k] = v;
        if (logs) logs[r * NH + k] = l;
      }
      ls[r] = (valid && !first) ? ls[r] + sum : sum;
    }
  }
}

template <int V> struct vec_of;
template <> struct vec_of<1> { using type = float; };
template <> struct vec_of<2> { using type = float2; };
template <> struct vec_of<4> { using type = float4; };

// X[r, col0 + i] = sum_j W[i*CC + j] * X[r, col0 + j] in place, one row per thread; V floats per access (4 where col0,
// CC and ldx are multiples of 4 and X is 16-byte aligned, else 2, else 1).  Rows past the item's length are written as 0.
template <int CC, int V>
__global__ __launch_bounds__(256) void mix_fwd_kernel(float* __restrict__ X, int ldx, int col0,
                                                      const float* __restrict__ W,
                                                      const int32_t* __restrict__ lens, long long rows, int T) {
  using vec = typename vec_of<V>::type;
  __shared__ float w[CC * CC];
  for (int i = threadIdx.x; i < CC * CC; i += blockDim.x) w[i] = W[i];
  __syncthreads();
  for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < rows;
       r += (long long)gridDim.x * blockDim.x) {
    float* xr = X + r * ldx + col0;
    union { vec v[CC / V]; float f[CC]; } in, out;
    if (row_valid(r, rows, lens, T)) {
#pragma unroll
      for (int q = 0; q < CC / V; ++q) in.v[q] = reinterpret_cast<const vec*>(xr)[q];
#pragma unroll
      for (int i = 0; i < CC; ++i) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < CC; ++j) a = fmaf(w[i * CC + j], in.f[j], a);
        out.f[i] = a;
      }
    } else {
#pragma unroll
      for (int i = 0; i < CC; ++i) out.f[i] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < CC / V; ++q) reinterpret_cast<vec*>(xr)[q] = out.v[q];
  }
}

// X[(b*Tg + g)*ldx + j] = audio[b*lda + g*ng + j] for g < lens[b], else 0 (a select: the samples past an item's length
// are never read).  V floats per thread and access: 4 where ng, ldx and lda are multiples of 4 and both arrays aligned.
template <int V>
__global__ __launch_bounds__(256) void group_audio_kernel(const float* __restrict__ audio, long long lda,
                                                          float* __restrict__ X, int ldx, int ng,
                                                          const int32_t* __restrict__ lens, int B, int Tg) {
  using vec = typename vec_of<V>::type;
  const int q = ng / V;
  const long long per = (long long)Tg * q;
  const long long total = (long long)B * per;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / per);
    const long long n = i - (long long)b * per;
    const int g = (int)(n / q), j = (int)(n - (long long)g * q) * V;
    vec v = vec();
    if (!lens || g < lens[b]) v = *reinterpret_cast<const vec*>(audio + b * lda + (long long)g * ng + j);
    *reinterpret_cast<vec*>(X + ((long long)b * Tg + g) * ldx + j) = v;
  }
}

// parts[b][0] = sum over the valid rows g < lens[b] of item b and the columns j < ng of X[(b*Tg + g)*ldx + j]^2,
// parts[b][1] = sum over the same rows of ls[b*Tg + g]; float64.  One workgroup per item and a fixed order: thread t sums
// rows t, t + 1024, .. in that order, the 64 lanes of a wave combine in an xor butterfly, thread 0 adds the 16 waves'
// sums in wave order.  No atomics, so two runs give the same bits and an item's sums do not depend on its neighbours.
constexpr int NLL_THREADS = 1024;
template <bool VEC>
__global__ __launch_bounds__(NLL_THREADS) void nll_parts_kernel(const float* __restrict__ X, int ldx, int ng,
                                                                const float* __restrict__ ls,
                                                                const int32_t* __restrict__ lens, int Tg,
                                                                double* __restrict__ parts) {
  __shared__ double sh[2][NLL_THREADS / 64];
  const int b = blockIdx.x;
  int len = lens ? lens[b] : Tg;
  len = len < 0 ? 0 : (len > Tg ? Tg : len);
  double sq = 0.0, sl = 0.0;
  for (int g = threadIdx.x; g < len; g += NLL_THREADS) {
    const long long r = (long long)b * Tg + g;
    const float* xr = X + r * ldx;
    double a = 0.0;
    if (VEC) {
      for (int j = 0; j < ng; j += 4) {
        const float4 v = *reinterpret_cast<const float4*>(xr + j);
        a += (double)v.x * v.x;
        a += (double)v.y * v.y;
        a += (double)v.z * v.z;
        a += (double)v.w * v.w;
      }
    } else {
      for (int j = 0; j < ng; ++j) a += (double)xr[j] * xr[j];
    }
    sq += a;
    sl += (double)ls[r];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_xor(sq, o, 64);
    sl += __shfl_xor(sl, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sh[0][wv] = sq;
    sh[1][wv] = sl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tq = 0.0, tl = 0.0;
    for (int i = 0; i < NLL_THREADS / 64; ++i) {
      tq += sh[0][i];
      tl += sh[1][i];
    }
    parts[2 * b] = tq;
    parts[2 * b + 1] = tl;
  }
}

// audio[b*lda + g*ng + j] = X[(b*Tg + g)*ldx + col0 + j] for g < lens[b], else 0 (every sample of [0, Tg*ng) written)
__global__ __launch_bounds__(256) void ungroup_kernel(const float* __restrict__ X, int ldx, int col0, int ng,
                                                      float* __restrict__ audio, long long lda,
                                                      const int32_t* __restrict__ lens, int B, int Tg) {
  const long long per = (long long)Tg * ng;
  const long long total = (long long)B * per;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / per);
    const long long n = i - (long long)b * per;
    const int g = (int)(n / ng), j = (int)(n - (long long)g * ng);
    const bool valid = !lens || g < lens[b];
    audio[b * lda + n] = valid ? X[((long long)b * Tg + g) * ldx + col0 + j] : 0.f;
  }
}

}  // namespace

extern "C" int radmmm_wg_group_cond(const float* up, int64_t up_item_stride, float* rows, int ldr, const int32_t* lens,
                                    int B, int Tg, int n_mel, int n_group, radmmm_stream_t stream) {
  RADMMM_REQUIRE(up && rows, "wg_group_cond: null pointer");
  RADMMM_REQUIRE(B > 0 && Tg > 0 && n_mel > 0 && n_group > 0 && ldr >= n_mel * n_group &&
                     up_item_stride >= (int64_t)Tg * n_group * n_mel && (int64_t)B * Tg <= 0x7fffffffLL,
                 "wg_group_cond: bad dims (B=%d Tg=%d n_mel=%d n_group=%d ldr=%d item_stride=%lld)", B, Tg, n_mel,
                 n_group, ldr, (long long)up_item_stride);
  const long long R = (long long)B * Tg;
  hipLaunchKernelGGL(group_cond_kernel, dim3(grid_for(R * ldr, 256)), dim3(256), 0, ST(stream), up,
                     (long long)up_item_stride, rows, ldr, lens, R, Tg, n_mel, n_group);
  return radmmm::check_launch("wg_group_cond");
}

extern "C" int radmmm_wg_noise_rows(const float* z, float sigma, float* X, int ldx, int col0, int ch,
                                    const int32_t* lens, int B, int Tg, radmmm_stream_t stream) {
  RADMMM_REQUIRE(z && X, "wg_noise_rows: null pointer");
  RADMMM_REQUIRE(B > 0 && Tg > 0 && ch > 0 && col0 >= 0 && col0 + ch <= ldx,
                 "wg_noise_rows: bad dims (B=%d Tg=%d ch=%d col0=%d ldx=%d)", B, Tg, ch, col0, ldx);
  hipLaunchKernelGGL(noise_rows_kernel, dim3(grid_for((long long)B * ch * Tg, 256)), dim3(256), 0, ST(stream), z, sigma,
                     X, ldx, col0, ch, lens, B, Tg);
  return radmmm::check_launch("wg_noise_rows");
}

extern "C" int radmmm_wg_start(const float* X, int ldx, int col0, int n_half, const float* W, const float* bias,
                               float* H, int ldh, int C, const int32_t* lens, int rows, int T,
                               radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && W && H, "wg_start: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && ldh % 4 == 0 && ldh >= C && n_half >= 1 &&
                     n_half <= START_MAX_NH && col0 >= 0 && col0 + n_half <= ldx,
                 "wg_start: bad dims (rows=%d T=%d C=%d ldh=%d n_half=%d col0=%d ldx=%d)", rows, T, C, ldh, n_half, col0,
                 ldx);
  RADMMM_REQUIRE(radmmm::aligned16(H), "wg_start: H must be 16B aligned");
  hipLaunchKernelGGL(start_kernel, dim3(grid_for((long long)rows * (C / 4), 256)), dim3(256), 0, ST(stream), X, ldx,
                     col0, n_half, W, bias, H, ldh, C, lens, (long long)rows, T);
  return radmmm::check_launch("wg_start");
}

extern "C" int radmmm_wg_gate(const float* a, int lda, const float* cond, int ldcond, int cond_off, float* y, int ldy,
                              int C, const int32_t* lens, int rows, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(a && cond && y, "wg_gate: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && lda % 4 == 0 && lda >= 2 * C &&
                     ldcond % 4 == 0 && cond_off >= 0 && cond_off % 4 == 0 && cond_off + 2 * C <= ldcond &&
                     ldy % 4 == 0 && ldy >= C,
                 "wg_gate: bad dims (rows=%d T=%d C=%d lda=%d ldcond=%d cond_off=%d ldy=%d)", rows, T, C, lda, ldcond,
                 cond_off, ldy);
  RADMMM_REQUIRE(radmmm::aligned16(a) && radmmm::aligned16(cond) && radmmm::aligned16(y),
                 "wg_gate: a / cond / y must be 16B aligned");
  hipLaunchKernelGGL(gate_kernel, dim3(grid_for((long long)rows * (C / 4), 256)), dim3(256), 0, ST(stream), a, lda, cond,
                     ldcond, cond_off, y, ldy, C, lens, (long long)rows, T);
  return radmmm::check_launch("wg_gate");
}

extern "C" int radmmm_wg_res_skip(const float* rs, int ldrs, float* H, int ldh, float* S, int lds, int C, int first,
                                  int last, const int32_t* lens, int rows, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(rs && S && (H || last), "wg_res_skip: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && ldrs % 4 == 0 &&
                     ldrs >= (last ? C : 2 * C) && lds % 4 == 0 && lds >= C && (last || (ldh % 4 == 0 && ldh >= C)),
                 "wg_res_skip: bad dims (rows=%d T=%d C=%d ldrs=%d ldh=%d lds=%d last=%d)", rows, T, C, ldrs, ldh, lds,
                 last);
  RADMMM_REQUIRE(radmmm::aligned16(rs) && radmmm::aligned16(S) && (last || radmmm::aligned16(H)),
                 "wg_res_skip: rs / H / S must be 16B aligned");
  hipLaunchKernelGGL(res_skip_kernel, dim3(grid_for((long long)rows * (C / 4), 256)), dim3(256), 0, ST(stream), rs, ldrs,
                     H, ldh, S, lds, C, first, last, lens, (long long)rows, T);
  return radmmm::check_launch("wg_res_skip");
}

extern "C" int radmmm_wg_start_split(const float* X, int ldx, int col0, int n_half, const float* W, const float* bias,
                                     float* H, int ldh, void* Hh, void* Hl, int ldp, int C, const int32_t* lens,
                                     int rows, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && W && H && Hh, "wg_start_split: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 8 == 0 && ldh % 4 == 0 && ldh >= C && ldp % 8 == 0 &&
                     ldp >= C && n_half >= 1 && n_half <= START_MAX_NH && col0 >= 0 && col0 + n_half <= ldx,
                 "wg_start_split: bad dims (rows=%d T=%d C=%d ldh=%d ldp=%d n_half=%d col0=%d ldx=%d; C, ldp %% 8 == 0)",
                 rows, T, C, ldh, ldp, n_half, col0, ldx);
  RADMMM_REQUIRE(radmmm::aligned16(H) && radmmm::aligned16(Hh) && radmmm::aligned16(Hl),
                 "wg_start_split: H / Hh / Hl must be 16B aligned");
  hipLaunchKernelGGL(start_split_kernel, dim3(grid_for((long long)rows * (ldp / 8), 256)), dim3(256), 0, ST(stream), X,
                     ldx, col0, n_half, W, bias, H, ldh, Hh, Hl, ldp, C, lens, (long long)rows, T);
  return radmmm::check_launch("wg_start_split");
}

extern "C" int radmmm_wg_gate_split(const float* a, int lda, const float* cond, int ldcond, int cond_off, void* yh,
                                    void* yl, int ldp, int C, const int32_t* lens, int rows, int T,
                                    radmmm_stream_t stream) {
  RADMMM_REQUIRE(a && cond && yh, "wg_gate_split: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 8 == 0 && lda % 4 == 0 && lda >= 2 * C &&
                     ldcond % 4 == 0 && cond_off >= 0 && cond_off % 4 == 0 && cond_off + 2 * C <= ldcond &&
                     ldp % 8 == 0 && ldp >= C,
                 "wg_gate_split: bad dims (rows=%d T=%d C=%d lda=%d ldcond=%d cond_off=%d ldp=%d; C, ldp %% 8 == 0)", rows,
                 T, C, lda, ldcond, cond_off, ldp);
  RADMMM_REQUIRE(radmmm::aligned16(a) && radmmm::aligned16(cond) && radmmm::aligned16(yh) && radmmm::aligned16(yl),
                 "wg_gate_split: a / cond / yh / yl must be 16B aligned");
  hipLaunchKernelGGL(gate_split_kernel, dim3(grid_for((long long)rows * (ldp / 8), 256)), dim3(256), 0, ST(stream), a,
                     lda, cond, ldcond, cond_off, yh, yl, ldp, C, lens, (long long)rows, T);
  return radmmm::check_launch("wg_gate_split");
}

extern "C" int radmmm_wg_res_skip_split(const float* rs, int ldrs, float* H, int ldh, float* S, int lds, void* Hh,
                                        void* Hl, int ldp, int C, int first, int last, const int32_t* lens, int rows,
                                        int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(rs && S && (last || (H && Hh)), "wg_res_skip_split: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 8 == 0 && ldrs % 4 == 0 &&
                     ldrs >= (last ? C : 2 * C) && lds % 4 == 0 && lds >= C &&
                     (last || (ldh % 4 == 0 && ldh >= C && ldp % 8 == 0 && ldp >= C)),
                 "wg_res_skip_split: bad dims (rows=%d T=%d C=%d ldrs=%d ldh=%d lds=%d ldp=%d last=%d; C, ldp %% 8 == 0)",
                 rows, T, C, ldrs, ldh, lds, ldp, last);
  RADMMM_REQUIRE(radmmm::aligned16(rs) && radmmm::aligned16(S) &&
                     (last || (radmmm::aligned16(H) && radmmm::aligned16(Hh) && radmmm::aligned16(Hl))),
                 "wg_res_skip_split: rs / H / S / Hh / Hl must be 16B aligned");
  hipLaunchKernelGGL(res_skip_split_kernel, dim3(grid_for((long long)rows * ((last ? C : ldp) / 8), 256)), dim3(256), 0,
                     ST(stream), rs, ldrs, H, ldh, S, lds, Hh, Hl, ldp, C, first, last, lens, (long long)rows, T);
  return radmmm::check_launch("wg_res_skip_split");
}

extern "C" int radmmm_wg_end_coupling(const float* S, int lds, const float* Wend, const float* bend, const float* Winv,
                                      float* X, int ldx, int col0, int n_half, int C, const int32_t* lens, int rows,
                                      int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(S && Wend && Winv && X, "wg_end_coupling: null pointer");
  const int NO = 2 * n_half;
  const long long smem = ((long long)NO * C + NO * NO + NO) * 4;
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && lds % 4 == 0 && lds >= C && n_half >= 1 &&
                     n_half <= 4 && col0 >= 0 && col0 + NO <= ldx && smem <= 32768,
                 "wg_end_coupling: bad dims (rows=%d T=%d C=%d lds=%d n_half=%d col0=%d ldx=%d; n_half <= 4, "
                 "(2 n_half)(C + 2 n_half + 1) <= 8192)", rows, T, C, lds, n_half, col0, ldx);
  RADMMM_REQUIRE(radmmm::aligned16(S) && radmmm::aligned16(Wend), "wg_end_coupling: S / Wend must be 16B aligned");
  const dim3 grid(grid_for(((long long)rows + 15) / 16, 1)), block(256);
#define WG_END(NOV)                                                                                                  \
  hipLaunchKernelGGL(end_coupling_kernel<NOV>, grid, block, (size_t)smem, ST(stream), S, lds, Wend, bend, Winv, X, ldx, \
                     col0, C, lens, (long long)rows, T)
  switch (NO) {
    case 2: WG_END(2); break;
    case 4: WG_END(4); break;
    case 6: WG_END(6); break;
    default: WG_END(8); break;
  }
#undef WG_END
  return radmmm::check_launch("wg_end_coupling");
}

extern "C" int radmmm_wg_ungroup(const float* X, int ldx, int col0, int n_group, float* audio, int64_t lda,
                                 const int32_t* lens, int B, int Tg, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && audio, "wg_ungroup: null pointer");
  RADMMM_REQUIRE(B > 0 && Tg > 0 && n_group > 0 && col0 >= 0 && col0 + n_group <= ldx &&
                     lda >= (int64_t)Tg * n_group,
                 "wg_ungroup: bad dims (B=%d Tg=%d n_group=%d col0=%d ldx=%d lda=%lld)", B, Tg, n_group, col0, ldx,
                 (long long)lda);
  hipLaunchKernelGGL(ungroup_kernel, dim3(grid_for((long long)B * Tg * n_group, 256)), dim3(256), 0, ST(stream), X, ldx,
                     col0, n_group, audio, (long long)lda, lens, B, Tg);
  return radmmm::check_launch("wg_ungroup");
}

extern "C" int radmmm_wg_group_audio(const float* audio, int64_t lda, float* X, int ldx, int n_group,
                                     const int32_t* lens, int B, int Tg, radmmm_stream_t stream) {
  RADMMM_REQUIRE(audio && X, "wg_group_audio: null pointer");
  RADMMM_REQUIRE(B > 0 && Tg > 0 && n_group > 0 && ldx >= n_group && lda >= (int64_t)Tg * n_group &&
                     (int64_t)B * Tg <= 0x7fffffffLL,
                 "wg_group_audio: bad dims (B=%d Tg=%d n_group=%d ldx=%d lda=%lld)", B, Tg, n_group, ldx,
                 (long long)lda);
  const bool v4 = n_group % 4 == 0 && ldx % 4 == 0 && lda % 4 == 0 && radmmm::aligned16(audio) && radmmm::aligned16(X);
  const long long total = (long long)B * Tg * (v4 ? n_group / 4 : n_group);
  if (v4)
    hipLaunchKernelGGL(group_audio_kernel<4>, dim3(grid_for(total, 256)), dim3(256), 0, ST(stream), audio,
                       (long long)lda, X, ldx, n_group, lens, B, Tg);
  else
    hipLaunchKernelGGL(group_audio_kernel<1>, dim3(grid_for(total, 256)), dim3(256), 0, ST(stream), audio,
                       (long long)lda, X, ldx, n_group, lens, B, Tg);
  return radmmm::check_launch("wg_group_audio");
}

extern "C" int radmmm_wg_mix_fwd(float* X, int ldx, int col0, int c, const float* W, const int32_t* lens, int rows,
                                 int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && W, "wg_mix_fwd: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && c >= 2 && c <= 8 && c % 2 == 0 && col0 >= 0 && col0 + c <= ldx,
                 "wg_mix_fwd: bad dims (rows=%d T=%d c=%d col0=%d ldx=%d; c even, 2 <= c <= 8)", rows, T, c, col0, ldx);
  const bool a16 = radmmm::aligned16(X);
  const int V = (a16 && ldx % 4 == 0 && col0 % 4 == 0 && c % 4 == 0)                                      ? 4
                : ((reinterpret_cast<uintptr_t>(X) & 7) == 0 && ldx % 2 == 0 && col0 % 2 == 0) ? 2
                                                                                                : 1;
  const dim3 grid(grid_for(rows, 256)), block(256);
#define WG_MIX(CV, VV) \
  hipLaunchKernelGGL((mix_fwd_kernel<CV, VV>), grid, block, 0, ST(stream), X, ldx, col0, W, lens, (long long)rows, T)
#define WG_MIX_V(CV)            \
  do {                          \
    if (V == 2) WG_MIX(CV, 2);  \
    else WG_MIX(CV, 1);         \
  } while (0)
  switch (c) {
    case 2: WG_MIX_V(2); break;
    case 4:
      if (V == 4) WG_MIX(4, 4);
      else WG_MIX_V(4);
      break;
    case 6: WG_MIX_V(6); break;
    default:
      if (V == 4) WG_MIX(8, 4);
      else WG_MIX_V(8);
      break;
  }
#undef WG_MIX_V
#undef WG_MIX
  return radmmm::check_launch("wg_mix_fwd");
}

extern "C" int radmmm_wg_end_coupling_fwd(const float* S, int lds, const float* Wend, const float* bend, float* X, int ldx,
                                          int col0, int n_half, int C, float* ls, int first, float* log_s,
                                          const int32_t* lens, int rows, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(S && Wend && X && ls, "wg_end_coupling_fwd: null pointer");
  const int NO = 2 * n_half;
  // the limit of wg_end_coupling, whose LDS also holds Winv: a model that runs one direction runs the other
  const long long smem_twin = ((long long)NO * C + NO * NO + NO) * 4;
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && lds % 4 == 0 && lds >= C && n_half >= 1 &&
                     n_half <= 4 && col0 >= 0 && col0 + NO <= ldx && smem_twin <= 32768,
                 "wg_end_coupling_fwd: bad dims (rows=%d T=%d C=%d lds=%d n_half=%d col0=%d ldx=%d; n_half <= 4, "
                 "(2 n_half)(C + 2 n_half + 1) <= 8192)", rows, T, C, lds, n_half, col0, ldx);
  RADMMM_REQUIRE(radmmm::aligned16(S) && radmmm::aligned16(Wend), "wg_end_coupling_fwd: S / Wend must be 16B aligned");
  const size_t smem = ((size_t)NO * C + NO) * 4;
  const dim3 grid(grid_for(((long long)rows + 15) / 16, 1)), block(256);
#define WG_END_FWD(NOV)                                                                                               \
  hipLaunchKernelGGL(end_coupling_fwd_kernel<NOV>, grid, block, smem, ST(stream), S, lds, Wend, bend, X, ldx, col0, C, \
                     ls, first, log_s, lens, (long long)rows, T)
  switch (NO) {
    case 2: WG_END_FWD(2); break;
    case 4: WG_END_FWD(4); break;
    case 6: WG_END_FWD(6); break;
    default: WG_END_FWD(8); break;
  }
#undef WG_END_FWD
  return radmmm::check_launch("wg_end_coupling_fwd");
}

extern "C" int radmmm_wg_nll_parts(const float* X, int ldx, int n_group, const float* ls, const int32_t* lens, int B,
                                   int Tg, double* parts, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && ls && parts, "wg_nll_parts: null pointer");
  RADMMM_REQUIRE(B > 0 && Tg > 0 && n_group > 0 && ldx >= n_group && (int64_t)B * Tg <= 0x7fffffffLL,
                 "wg_nll_parts: bad dims (B=%d Tg=%d n_group=%d ldx=%d)", B, Tg, n_group, ldx);
  RADMMM_REQUIRE((reinterpret_cast<uintptr_t>(parts) & 7) == 0, "wg_nll_parts: parts must be 8B aligned");
  if (n_group % 4 == 0 && ldx % 4 == 0 && radmmm::aligned16(X))
    hipLaunchKernelGGL(nll_parts_kernel<true>, dim3(B), dim3(NLL_THREADS), 0, ST(stream), X, ldx, n_group, ls, lens, Tg,
                       parts);
  else
    hipLaunchKernelGGL(nll_parts_kernel<false>, dim3(B), dim3(NLL_THREADS), 0, ST(stream), X, ldx, n_group, ls, lens,
                       Tg, parts);
  return radmmm::check_launch("wg_nll_parts");
}

// ---- the backward pass of the audio -> latent direction ------------------------------------------------------------
// What the row GEMMs, radmmm_wgrad_f32 and radmmm_colsum do not cover.  Rows at or past an item's length are never read
// and every gradient row there is written as 0, so the GEMMs that follow may read all rows.  No atomics: the row
// reductions (wg_outer_reduce) leave one partial per 256-row tile, summed in tile order by radmmm_colsum_final.
namespace {

// o = Wend S[r] + bend recomputed as the forward does (end_dot), b = o[:NH], log_s = o[NH:], x1 the saved coupling input:
//   d_b = dX1', d_log_s = dX1' * exp(log_s) * x1 + g_ls, dX1 = dX1' * exp(log_s) (in place), dO[r] = [d_b, d_log_s],
//   dS[r, :] = Wend^T dO[r].  g_ls: one value for every row (ldg == 0) or [rows][ldg].
template <int NO>
__global__ __launch_bounds__(256) void coupling_bwd_kernel(const float* __restrict__ S, int lds,
                                                           const float* __restrict__ Wend,
                                                           const float* __restrict__ bend,
                                                           const float* __restrict__ Xs, int ldxs, float* __restrict__ dX,
                                                           int ldx, int col0, int C, const float* __restrict__ gls,
                                                           int ldg, float* __restrict__ dO, float* __restrict__ dS,
                                                           int ldds, const int32_t* __restrict__ lens, long long rows,
                                                           int T) {
  extern __shared__ __align__(16) float sh[];
  float* w = sh;                    // [NO][C]
  float* be = sh + NO * C;          // [NO]
  for (int i = threadIdx.x; i < NO * C; i += blockDim.x) w[i] = Wend[i];
  for (int i = threadIdx.x; i < NO; i += blockDim.x) be[i] = bend ? bend[i] : 0.f;
  __syncthreads();
  constexpr int NH = NO / 2;
  const int sub = threadIdx.x & 15, rloc = threadIdx.x >> 4;
  for (long long r0 = blockIdx.x * 16LL; r0 < rows; r0 += gridDim.x * 16LL) {
    const long long r = r0 + rloc;
    const bool valid = row_valid(r, rows, lens, T);
    float acc[NO];
    end_dot<NO>(S, lds, w, C, r, valid, sub, acc);
    float d[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) d[o] = 0.f;
    if (valid) {
      // every lane of the row computes the same NO values (a few loads that hit the same cache line)
      const float* x1 = Xs + r * ldxs + col0 + NH;
      const float* g1 = dX + r * ldx + col0 + NH;
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        const float e = expf(acc[NH + k] + be[NH + k]);
        const float g = g1[k];
        d[k] = g;
        d[NH + k] = fmaf(g * e, x1[k], ldg ? gls[r * ldg + k] : gls[0]);
      }
    }
    if (r < rows) {
      float* dsr = dS + r * ldds;
      for (int c = sub * 4; c < C; c += 64) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int o = 0; o < NO; ++o) {
          const float4 ww = *reinterpret_cast<const float4*>(w + o * C + c);
          v.x = fmaf(ww.x, d[o], v.x);
          v.y = fmaf(ww.y, d[o], v.y);
          v.z = fmaf(ww.z, d[o], v.z);
          v.w = fmaf(ww.w, d[o], v.w);
        }
        *reinterpret_cast<float4*>(dsr + c) = v;
      }
    }
    __syncthreads();   // every lane of a row has read dX1' before lane 0 overwrites it (uniform trip count: r0 is per block)
    if (sub == 0 && r < rows) {
      float* g1 = dX + r * ldx + col0 + NH;
#pragma unroll
      for (int k = 0; k < NH; ++k) g1[k] = valid ? d[k] * expf(acc[NH + k] + be[NH + k]) : 0.f;
#pragma unroll
      for (int o = 0; o < NO; ++o) dO[r * NO + o] = d[o];
    }
  }
}

__device__ __forceinline__ void gate_bwd1(float ta, float tc, float sa, float sc, float g, float& dt, float& ds) {
  const float t = tanhf(ta + tc), s = 1.f / (1.f + expf(-(sa + sc)));
  dt = g * s * (1.f - t * t);
  ds = g * t * s * (1.f - s);
}

// dA[r, c] = g[r, c] * sig * (1 - tanh^2), dA[r, C + c] = g[r, c] * tanh * sig * (1 - sig) of the gate's inputs
// a[r, :] + cond[r, off:]; 0 in the rows past an item's length (a / cond / g are not read there)
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ a, int lda,
                                                       const float* __restrict__ cond, int ldcond, int off,
                                                       const float* __restrict__ g, int ldg, float* __restrict__ dA,
                                                       int ldda, int C, const int32_t* __restrict__ lens,
                                                       long long rows, int T) {
  const int q = C >> 2;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 4;
    float4 dt = make_float4(0.f, 0.f, 0.f, 0.f), ds = dt;
    if (row_valid(r, rows, lens, T)) {
      const float* ar = a + r * lda + c;
      const float* cr = cond + r * ldcond + off + c;
      const float4 ta = *reinterpret_cast<const float4*>(ar), sa = *reinterpret_cast<const float4*>(ar + C);
      const float4 tc = *reinterpret_cast<const float4*>(cr), sc = *reinterpret_cast<const float4*>(cr + C);
      const float4 gv = *reinterpret_cast<const float4*>(g + r * ldg + c);
      gate_bwd1(ta.x, tc.x, sa.x, sc.x, gv.x, dt.x, ds.x);
      gate_bwd1(ta.y, tc.y, sa.y, sc.y, gv.y, dt.y, ds.y);
      gate_bwd1(ta.z, tc.z, sa.z, sc.z, gv.z, dt.z, ds.z);
      gate_bwd1(ta.w, tc.w, sa.w, sc.w, gv.w, dt.w, ds.w);
    }
    float* dr = dA + r * ldda + c;
    *reinterpret_cast<float4*>(dr) = dt;
    *reinterpret_cast<float4*>(dr + C) = ds;
  }
}

// ---- the two gradient producers of train_precision "h3" ---------------------------------------------------------------
// coupling_bwd_kernel / gate_bwd_kernel that also write the split f16 pair of scale * value (split_pack.h: the bits of
// radmmm_split_f16 of the fp32 output) in the pass that computes it: the A operand of the data-gradient GEMM and the GY
// operand of the weight gradient.  The conventions of the forward *_split kernels: a thread owns 8 columns of a row, one
// 16-byte store per half array; rows at or past an item's length and the padding columns up to pcols are zeros in both
// halves; the fp32 arithmetic is the twin's, operation for operation.  max |scale * value| is tracked per lane and the
// saturation flag is raised once per wave after the loop (raise_sat_flag): the only atomic, and nothing reads it here.

template <int NO>
__global__ __launch_bounds__(256) void coupling_bwd_split_kernel(
    const float* __restrict__ S, int lds, const float* __restrict__ Wend, const float* __restrict__ bend,
    const float* __restrict__ Xs, int ldxs, float* __restrict__ dX, int ldx, int col0, int C,
    const float* __restrict__ gls, int ldg, float* __restrict__ dO, float* __restrict__ dS, int ldds,
    void* __restrict__ Ph, void* __restrict__ Pl, int ldp, int pcols, float scale, int* __restrict__ sat_flag,
    const int32_t* __restrict__ lens, long long rows, int T) {
  extern __shared__ __align__(16) float sh[];
  float* w = sh;                    // [NO][C]
  float* be = sh + NO * C;          // [NO]
  for (int i = threadIdx.x; i < NO * C; i += blockDim.x) w[i] = Wend[i];
  for (int i = threadIdx.x; i < NO; i += blockDim.x) be[i] = bend ? bend[i] : 0.f;
  __syncthreads();
  constexpr int NH = NO / 2;
  const int sub = threadIdx.x & 15, rloc = threadIdx.x >> 4;
  float sat = 0.f;
  for (long long r0 = blockIdx.x * 16LL; r0 < rows; r0 += gridDim.x * 16LL) {
    const long long r = r0 + rloc;
    const bool valid = row_valid(r, rows, lens, T);
    float acc[NO];
    end_dot<NO>(S, lds, w, C, r, valid, sub, acc);
    float d[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) d[o] = 0.f;
    if (valid) {
      const float* x1 = Xs + r * ldxs + col0 + NH;
      const float* g1 = dX + r * ldx + col0 + NH;
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        const float e = expf(acc[NH + k] + be[NH + k]);
        const float g = g1[k];
        d[k] = g;
        d[NH + k] = fmaf(g * e, x1[k], ldg ? gls[r * ldg + k] : gls[0]);
      }
    }
    if (r < rows) {
      float* dsr = dS + r * ldds;
      for (int c = sub * 8; c < pcols; c += 128) {
        float v[8];
        zero8(v);
        if (c < C) {
#pragma unroll
          for (int o = 0; o < NO; ++o) {
            float ww[8];
            load8(w + o * C + c, ww);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaf(ww[e], d[o], v[e]);
          }
          store8(dsr + c, v);
        }
        sat = fmaxf(sat, radmmm::store_split8_f16_amax(Ph, Pl, r * ldp, c, scale, v));
      }
    }
    __syncthreads();   // every lane of a row has read dX1' before lane 0 overwrites it (uniform trip count: r0 is per block)
    if (sub == 0 && r < rows) {
      float* g1 = dX + r * ldx + col0 + NH;
#pragma unroll
      for (int k = 0; k < NH; ++k) g1[k] = valid ? d[k] * expf(acc[NH + k] + be[NH + k]) : 0.f;
#pragma unroll
      for (int o = 0; o < NO; ++o) dO[r * NO + o] = d[o];
    }
  }
  radmmm::raise_sat_flag(sat_flag, sat);
}

// thread i of a row: 8 columns c of the C gate channels (dt -> columns c, ds -> columns C + c of dA and of the pair), or,
// past them, 8 padding columns of the pair
__global__ __launch_bounds__(256) void gate_bwd_split_kernel(
    const float* __restrict__ a, int lda, const float* __restrict__ cond, int ldcond, int off,
    const float* __restrict__ g, int ldg, float* __restrict__ dA, int ldda, void* __restrict__ Ph,
    void* __restrict__ Pl, int ldp, int pcols, int C, float scale, int* __restrict__ sat_flag,
    const int32_t* __restrict__ lens, long long rows, int T) {
  const int qc = C >> 3, q = qc + ((pcols - 2 * C) >> 3);
  const long long total = rows * q;
  float sat = 0.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int j = (int)(i - r * q);
    float dt[8], ds[8];
    zero8(dt);
    zero8(ds);
    if (j < qc) {
      const int c = j * 8;
      if (row_valid(r, rows, lens, T)) {
        float ta[8], sa[8], tc[8], sc[8], gv[8];
        const float* ar = a + r * lda + c;
        const float* cr = cond + r * ldcond + off + c;
        load8(ar, ta);
        load8(ar + C, sa);
        load8(cr, tc);
        load8(cr + C, sc);
        load8(g + r * ldg + c, gv);
#pragma unroll
        for (int e = 0; e < 8; ++e) gate_bwd1(ta[e], tc[e], sa[e], sc[e], gv[e], dt[e], ds[e]);
      }
      float* dr = dA + r * ldda + c;
      store8(dr, dt);
      store8(dr + C, ds);
      sat = fmaxf(sat, radmmm::store_split8_f16_amax(Ph, Pl, r * ldp, c, scale, dt));
      sat = fmaxf(sat, radmmm::store_split8_f16_amax(Ph, Pl, r * ldp, C + c, scale, ds));
    } else {
      radmmm::store_split8_f16(Ph, Pl, r * ldp, 2 * C + (j - qc) * 8, scale, dt);
    }
  }
  radmmm::raise_sat_flag(sat_flag, sat);
}

// dX[r, col0 + i] += sum_c Wt[i*C + c] * dH[r, c], i < NH (Wt = the start weight transposed, in LDS): end_dot's sum
template <int NH>
__global__ __launch_bounds__(256) void start_bwd_kernel(const float* __restrict__ dH, int ldh,
                                                        const float* __restrict__ Wt, float* __restrict__ dX, int ldx,
                                                        int col0, int C, const int32_t* __restrict__ lens,
                                                        long long rows, int T) {
  extern __shared__ __align__(16) float sh[];
  for (int i = threadIdx.x; i < NH * C; i += blockDim.x) sh[i] = Wt[i];
  __syncthreads();
  const int sub = threadIdx.x & 15, rloc = threadIdx.x >> 4;
  for (long long r0 = blockIdx.x * 16LL; r0 < rows; r0 += gridDim.x * 16LL) {
    const long long r = r0 + rloc;
    const bool valid = row_valid(r, rows, lens, T);
    float acc[NH];
    end_dot<NH>(dH, ldh, sh, C, r, valid, sub, acc);
    if (sub == 0 && valid) {
      float* xr = dX + r * ldx + col0;
#pragma unroll
      for (int i = 0; i < NH; ++i) xr[i] += acc[i];
    }
  }
}

// part[(tile*M + m)*N + n] = sum over the valid rows r of the 256-row tile of A[r*lda + m] * B[r*ldb + n] (A == NULL:
// M = 1 and A = 1, a column sum).  A thread owns one column n and M <= 8 accumulators; with N < 256 the 256 / NB row
// subsets of a tile (NB = N rounded up to a power of two) are added in subset order through LDS.
constexpr int OR_TILE = 256, OR_MAX_M = 8;
__global__ __launch_bounds__(256) void outer_reduce_kernel(const float* __restrict__ A, int lda, int M,
                                                           const float* __restrict__ Bm, int ldb, int N, int NB,
                                                           float* __restrict__ part,
                                                           const int32_t* __restrict__ lens, long long rows, int T) {
  __shared__ float red[256 * OR_MAX_M];
  const int RS = 256 / NB;
  const int nl = threadIdx.x % NB, rsub = threadIdx.x / NB;
  const int n = blockIdx.y * NB + nl;
  const long long tile0 = (long long)blockIdx.x * OR_TILE;
  float acc[OR_MAX_M];
#pragma unroll
  for (int m = 0; m < OR_MAX_M; ++m) acc[m] = 0.f;
  if (n < N) {
    for (int k = rsub; k < OR_TILE; k += RS) {
      const long long r = tile0 + k;
      if (!row_valid(r, rows, lens, T)) continue;
      const float b = Bm[r * ldb + n];
      if (A) {
        const float* ar = A + r * lda;
#pragma unroll
        for (int m = 0; m < OR_MAX_M; ++m)
          if (m < M) acc[m] = fmaf(ar[m], b, acc[m]);
      } else {
        acc[0] += b;
      }
    }
  }
  if (RS > 1) {
#pragma unroll
    for (int m = 0; m < OR_MAX_M; ++m) red[(rsub * OR_MAX_M + m) * NB + nl] = acc[m];
    __syncthreads();
    if (rsub == 0) {
#pragma unroll
      for (int m = 0; m < OR_MAX_M; ++m) {
        float s = 0.f;
        for (int q = 0; q < RS; ++q) s += red[(q * OR_MAX_M + m) * NB + nl];
        acc[m] = s;
      }
    }
  }
  if (rsub == 0 && n < N) {
#pragma unroll
    for (int m = 0; m < OR_MAX_M; ++m)
      if (m < M) part[((long long)blockIdx.x * M + m) * N + n] = acc[m];
  }
}

// per flow k (one thread each): Winv = W^-1 (fp32) and logdet[k] = log|det W| by Gauss-Jordan elimination with partial
// pivoting in float64; W is c x c, c <= 8, flow k's matrix at offs[k] floats in both packed arrays
struct inv_plan { int n; int c[32]; int off[32]; };
__global__ void inv_logdet_kernel(const float* __restrict__ W, inv_plan plan, float* __restrict__ Winv,
                                  double* __restrict__ logdet) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= plan.n) return;
  const int c = plan.c[k];
  const float* w = W + plan.off[k];
  double a[8][16];
  for (int i = 0; i < c; ++i)
    for (int j = 0; j < c; ++j) {
      a[i][j] = (double)w[i * c + j];
      a[i][c + j] = i == j ? 1.0 : 0.0;
    }
  double ld = 0.0;
  for (int p = 0; p < c; ++p) {
    int best = p;
    for (int i = p + 1; i < c; ++i)
      if (fabs(a[i][p]) > fabs(a[best][p])) best = i;
    if (best != p)
      for (int j = 0; j < 2 * c; ++j) {
        const double t = a[p][j];
        a[p][j] = a[best][j];
        a[best][j] = t;
      }
    const double piv = a[p][p];
    ld += log(fabs(piv));
    for (int j = 0; j < 2 * c; ++j) a[p][j] /= piv;
    for (int i = 0; i < c; ++i) {
      if (i == p) continue;
      const double f = a[i][p];
      for (int j = 0; j < 2 * c; ++j) a[i][j] -= f * a[p][j];
    }
  }
  float* o = Winv + plan.off[k];
  for (int i = 0; i < c; ++i)
    for (int j = 0; j < c; ++j) o[i * c + j] = (float)a[i][c + j];
  logdet[k] = ld;
}

// the inverse permutation of group_cond_kernel: up[b*item_stride + (g*ng + j)*n_mel + m] = rows[(b*Tg + g)*ldr + m*ng + j]
// for g < lens[b], else 0 (rows past an item's length are not read)
__global__ __launch_bounds__(256) void ungroup_cond_kernel(const float* __restrict__ rows, int ldr,
                                                           float* __restrict__ up, long long item_stride,
                                                           const int32_t* __restrict__ lens, long long R, int Tg,
                                                           int n_mel, int ng) {
  const int cols = n_mel * ng;
  const long long total = R * cols;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / cols;
    const int c = (int)(i - r * cols);             // = j*n_mel + m: the order of the destination
    const int j = c / n_mel, m = c - j * n_mel;
    const int b = (int)(r / Tg), g = (int)(r - (long long)b * Tg);
    const bool valid = !lens || g < lens[b];
    up[b * item_stride + (long long)g * cols + c] = valid ? rows[r * ldr + m * ng + j] : 0.f;
  }
}

}  // namespace

extern "C" int radmmm_wg_coupling_bwd(const float* S, int lds, const float* Wend, const float* bend, const float* Xs,
                                      int ldxs, float* dX, int ldx, int col0, int n_half, int C, const float* g_ls,
                                      int ldg, float* dO, float* dS, int ldds, const int32_t* lens, int rows, int T,
                                      radmmm_stream_t stream) {
  RADMMM_REQUIRE(S && Wend && Xs && dX && g_ls && dO && dS, "wg_coupling_bwd: null pointer");
  const int NO = 2 * n_half;
  const long long smem_twin = ((long long)NO * C + NO * NO + NO) * 4;   // the limit of the forward kernels
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && lds % 4 == 0 && lds >= C &&
                     ldds % 4 == 0 && ldds >= C && n_half >= 1 && n_half <= 4 && col0 >= 0 && col0 + NO <= ldx &&
                     col0 + NO <= ldxs && (ldg == 0 || ldg >= n_half) && smem_twin <= 32768,
                 "wg_coupling_bwd: bad dims (rows=%d T=%d C=%d lds=%d ldds=%d n_half=%d col0=%d ldx=%d ldxs=%d ldg=%d)",
                 rows, T, C, lds, ldds, n_half, col0, ldx, ldxs, ldg);
  RADMMM_REQUIRE(radmmm::aligned16(S) && radmmm::aligned16(Wend) && radmmm::aligned16(dS),
                 "wg_coupling_bwd: S / Wend / dS must be 16B aligned");
  const size_t smem = ((size_t)NO * C + NO) * 4;
  const dim3 grid(grid_for(((long long)rows + 15) / 16, 1)), block(256);
#define WG_CPL_BWD(NOV)                                                                                              \
  hipLaunchKernelGGL(coupling_bwd_kernel<NOV>, grid, block, smem, ST(stream), S, lds, Wend, bend, Xs, ldxs, dX, ldx, \
                     col0, C, g_ls, ldg, dO, dS, ldds, lens, (long long)rows, T)
  switch (NO) {
    case 2: WG_CPL_BWD(2); break;
    case 4: WG_CPL_BWD(4); break;
    case 6: WG_CPL_BWD(6); break;
    default: WG_CPL_BWD(8); break;
  }
#undef WG_CPL_BWD
  return radmmm::check_launch("wg_coupling_bwd");
}

extern "C" int radmmm_wg_gate_bwd(const float* a, int lda, const float* cond, int ldcond, int cond_off, const float* g,
                                  int ldg, float* dA, int ldda, int C, const int32_t* lens, int rows, int T,
                                  radmmm_stream_t stream) {
  RADMMM_REQUIRE(a && cond && g && dA, "wg_gate_bwd: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && lda % 4 == 0 && lda >= 2 * C &&
                     ldcond % 4 == 0 && cond_off >= 0 && cond_off % 4 == 0 && cond_off + 2 * C <= ldcond &&
                     ldg % 4 == 0 && ldg >= C && ldda % 4 == 0 && ldda >= 2 * C,
                 "wg_gate_bwd: bad dims (rows=%d T=%d C=%d lda=%d ldcond=%d cond_off=%d ldg=%d ldda=%d)", rows, T, C, lda,
                 ldcond, cond_off, ldg, ldda);
  RADMMM_REQUIRE(radmmm::aligned16(a) && radmmm::aligned16(cond) && radmmm::aligned16(g) && radmmm::aligned16(dA),
                 "wg_gate_bwd: a / cond / g / dA must be 16B aligned");
  hipLaunchKernelGGL(gate_bwd_kernel, dim3(grid_for((long long)rows * (C / 4), 256)), dim3(256), 0, ST(stream), a, lda,
                     cond, ldcond, cond_off, g, ldg, dA, ldda, C, lens, (long long)rows, T);
  return radmmm::check_launch("wg_gate_bwd");
}

extern "C" int radmmm_wg_coupling_bwd_split(const float* S, int lds, const float* Wend, const float* bend, const float* Xs,
                                            int ldxs, float* dX, int ldx, int col0, int n_half, int C, const float* g_ls,
                                            int ldg, float* dO, float* dS, int ldds, void* dSh, void* dSl, int ldp,
                                            int pcols, float scale, int32_t* sat_flag, const int32_t* lens, int rows,
                                            int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(S && Wend && Xs && dX && g_ls && dO && dS && dSh && dSl, "wg_coupling_bwd_split: null pointer");
  const int NO = 2 * n_half;
  const long long smem_twin = ((long long)NO * C + NO * NO + NO) * 4;   // the limit of the forward kernels
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 8 == 0 && lds % 4 == 0 && lds >= C &&
                     ldds % 4 == 0 && ldds >= C && n_half >= 1 && n_half <= 4 && col0 >= 0 && col0 + NO <= ldx &&
                     col0 + NO <= ldxs && (ldg == 0 || ldg >= n_half) && smem_twin <= 32768 && ldp % 8 == 0 &&
                     pcols % 8 == 0 && pcols >= C && ldp >= pcols,
                 "wg_coupling_bwd_split: bad dims (rows=%d T=%d C=%d lds=%d ldds=%d n_half=%d col0=%d ldx=%d ldxs=%d ldg=%d "
                 "ldp=%d pcols=%d; C, ldp, pcols %% 8 == 0, C <= pcols <= ldp)",
                 rows, T, C, lds, ldds, n_half, col0, ldx, ldxs, ldg, ldp, pcols);
  RADMMM_REQUIRE(radmmm::aligned16(S) && radmmm::aligned16(Wend) && radmmm::aligned16(dS) && radmmm::aligned16(dSh) &&
                     radmmm::aligned16(dSl),
                 "wg_coupling_bwd_split: S / Wend / dS / dSh / dSl must be 16B aligned");
  const size_t smem = ((size_t)NO * C + NO) * 4;
  const dim3 grid(grid_for(((long long)rows + 15) / 16, 1)), block(256);
#define WG_CPL_BWD_SPLIT(NOV)                                                                                          \
  hipLaunchKernelGGL(coupling_bwd_split_kernel<NOV>, grid, block, smem, ST(stream), S, lds, Wend, bend, Xs, ldxs, dX, \
                     ldx, col0, C, g_ls, ldg, dO, dS, ldds, dSh, dSl, ldp, pcols, scale, sat_flag, lens,              \
                     (long long)rows, T)
  switch (NO) {
    case 2: WG_CPL_BWD_SPLIT(2); break;
    case 4: WG_CPL_BWD_SPLIT(4); break;
    case 6: WG_CPL_BWD_SPLIT(6); break;
    default: WG_CPL_BWD_SPLIT(8); break;
  }
#undef WG_CPL_BWD_SPLIT
  return radmmm::check_launch("wg_coupling_bwd_split");
}

extern "C" int radmmm_wg_gate_bwd_split(const float* a, int lda, const float* cond, int ldcond, int cond_off,
                                        const float* g, int ldg, float* dA, int ldda, void* dAh, void* dAl, int ldp,
                                        int pcols, int C, float scale, int32_t* sat_flag, const int32_t* lens, int rows,
                                        int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(a && cond && g && dA && dAh && dAl, "wg_gate_bwd_split: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 8 == 0 && lda % 4 == 0 && lda >= 2 * C &&
                     ldcond % 4 == 0 && cond_off >= 0 && cond_off % 4 == 0 && cond_off + 2 * C <= ldcond &&
                     ldg % 4 == 0 && ldg >= C && ldda % 4 == 0 && ldda >= 2 * C && ldp % 8 == 0 && pcols % 8 == 0 &&
                     pcols >= 2 * C && ldp >= pcols,
                 "wg_gate_bwd_split: bad dims (rows=%d T=%d C=%d lda=%d ldcond=%d cond_off=%d ldg=%d ldda=%d ldp=%d "
                 "pcols=%d; C, ldp, pcols %% 8 == 0, 2 C <= pcols <= ldp)",
                 rows, T, C, lda, ldcond, cond_off, ldg, ldda, ldp, pcols);
  RADMMM_REQUIRE(radmmm::aligned16(a) && radmmm::aligned16(cond) && radmmm::aligned16(g) && radmmm::aligned16(dA) &&
                     radmmm::aligned16(dAh) && radmmm::aligned16(dAl),
                 "wg_gate_bwd_split: a / cond / g / dA / dAh / dAl must be 16B aligned");
  hipLaunchKernelGGL(gate_bwd_split_kernel, dim3(grid_for((long long)rows * ((pcols - C) / 8), 256)), dim3(256), 0,
                     ST(stream), a, lda, cond, ldcond, cond_off, g, ldg, dA, ldda, dAh, dAl, ldp, pcols, C, scale,
                     sat_flag, lens, (long long)rows, T);
  return radmmm::check_launch("wg_gate_bwd_split");
}

extern "C" int radmmm_wg_start_bwd(const float* dH, int ldh, const float* Wt, float* dX, int ldx, int col0, int n_half,
                                   int C, const int32_t* lens, int rows, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dH && Wt && dX, "wg_start_bwd: null pointer");
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && C > 0 && C % 4 == 0 && ldh % 4 == 0 && ldh >= C && n_half >= 1 &&
                     n_half <= 4 && col0 >= 0 && col0 + n_half <= ldx && (long long)n_half * C * 4 <= 32768,
                 "wg_start_bwd: bad dims (rows=%d T=%d C=%d ldh=%d n_half=%d col0=%d ldx=%d)", rows, T, C, ldh, n_half,
                 col0, ldx);
  RADMMM_REQUIRE(radmmm::aligned16(dH) && radmmm::aligned16(Wt), "wg_start_bwd: dH / Wt must be 16B aligned");
  const size_t smem = (size_t)n_half * C * 4;
  const dim3 grid(grid_for(((long long)rows + 15) / 16, 1)), block(256);
#define WG_START_BWD(NHV)                                                                                          \
  hipLaunchKernelGGL(start_bwd_kernel<NHV>, grid, block, smem, ST(stream), dH, ldh, Wt, dX, ldx, col0, C, lens, \
                     (long long)rows, T)
  switch (n_half) {
    case 1: WG_START_BWD(1); break;
    case 2: WG_START_BWD(2); break;
    case 3: WG_START_BWD(3); break;
    default: WG_START_BWD(4); break;
  }
#undef WG_START_BWD
  return radmmm::check_launch("wg_start_bwd");
}

extern "C" int64_t radmmm_wg_outer_reduce_scratch_floats(int rows, int M, int N) {
  return ((int64_t)rows + OR_TILE - 1) / OR_TILE * (int64_t)(M > 0 ? M : 1) * N;
}

extern "C" int radmmm_wg_outer_reduce(const float* A, int lda, int M, const float* B, int ldb, int N, float* out,
                                      float* scratch, const int32_t* lens, int rows, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(B && out && scratch, "wg_outer_reduce: null pointer");
  if (!A) M = 1;
  RADMMM_REQUIRE(rows > 0 && T > 0 && rows % T == 0 && M >= 1 && M <= OR_MAX_M && N >= 1 && ldb >= N && (!A || lda >= M) &&
                     (long long)M * N <= 0x7fffffffLL,
                 "wg_outer_reduce: bad dims (rows=%d T=%d M=%d N=%d lda=%d ldb=%d; M <= 8)", rows, T, M, N, lda, ldb);
  int NB = 1;
  while (NB < N && NB < 256) NB <<= 1;
  const int tiles = (rows + OR_TILE - 1) / OR_TILE;
  RADMMM_REQUIRE((N + NB - 1) / NB <= 65535, "wg_outer_reduce: N=%d too wide", N);
  hipLaunchKernelGGL(outer_reduce_kernel, dim3(tiles, (N + NB - 1) / NB), dim3(256), 0, ST(stream), A, lda, M, B, ldb, N,
                     NB, scratch, lens, (long long)rows, T);
  const int rc = radmmm::check_launch("wg_outer_reduce");
  if (rc) return rc;
  return radmmm_colsum_final(scratch, out, tiles, M * N, stream);
}

extern "C" int radmmm_wg_inv_logdet(const float* W, const int32_t* cs, int n, float* Winv, double* logdet,
                                    radmmm_stream_t stream) {
  RADMMM_REQUIRE(W && cs && Winv && logdet, "wg_inv_logdet: null pointer");
  RADMMM_REQUIRE(n >= 1 && n <= 32, "wg_inv_logdet: n=%d flows (1 .. 32)", n);
  RADMMM_REQUIRE((reinterpret_cast<uintptr_t>(logdet) & 7) == 0, "wg_inv_logdet: logdet must be 8B aligned");
  inv_plan plan;
  plan.n = n;
  int off = 0;
  for (int k = 0; k < n; ++k) {
    RADMMM_REQUIRE(cs[k] >= 1 && cs[k] <= 8, "wg_inv_logdet: matrix %d is %d x %d (1 .. 8)", k, cs[k], cs[k]);
    plan.c[k] = cs[k];
    plan.off[k] = off;
    off += cs[k] * cs[k];
  }
  for (int k = n; k < 32; ++k) plan.c[k] = plan.off[k] = 0;
  hipLaunchKernelGGL(inv_logdet_kernel, dim3(1), dim3(64), 0, ST(stream), W, plan, Winv, logdet);
  return radmmm::check_launch("wg_inv_logdet");
}

extern "C" int radmmm_wg_ungroup_cond(const float* rows, int ldr, float* up, int64_t up_item_stride, const int32_t* lens,
                                      int B, int Tg, int n_mel, int n_group, radmmm_stream_t stream) {
  RADMMM_REQUIRE(up && rows, "wg_ungroup_cond: null pointer");
  RADMMM_REQUIRE(B > 0 && Tg > 0 && n_mel > 0 && n_group > 0 && ldr >= n_mel * n_group &&
                     up_item_stride >= (int64_t)Tg * n_group * n_mel && (int64_t)B * Tg <= 0x7fffffffLL,
                 "wg_ungroup_cond: bad dims (B=%d Tg=%d n_mel=%d n_group=%d ldr=%d item_stride=%lld)", B, Tg, n_mel,
                 n_group, ldr, (long long)up_item_stride);
  const long long R = (long long)B * Tg;
  hipLaunchKernelGGL(ungroup_cond_kernel, dim3(grid_for(R * n_mel * n_group, 256)), dim3(256), 0, ST(stream), rows, ldr,
                     up, (long long)up_item_stride, lens, R, Tg, n_mel, n_group);
  return radmmm::check_launch("wg_ungroup_cond");
}
