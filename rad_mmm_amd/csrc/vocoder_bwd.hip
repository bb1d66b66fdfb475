// Backward pass of the HiFi-GAN generator on gfx950: the two audio-rate kernels that the row GEMMs (data gradients),
// radmmm_wgrad_f32 (weight gradients) and radmmm_colsum (bias gradients) do not cover.  Same channels-last row layout
// and per-item length masking as csrc/vocoder.hip: rows at or past an item's length are never read and are written
// as zeros.  Both kernels are bandwidth-bound: one float4 per access, every sum in a fixed order, no atomics.
//   radmmm_voc_lrelu_bwd      gx = [gx +] gy * leaky_relu'(x / div) from the saved output a = leaky_relu(x / div)
//   radmmm_voc_conv_post_bwd  backward of conv_post + tanh: dx through the taps and leaky_relu(x / div), dw and dbias
//                             from a two-stage reduction (one partial row per workgroup, added in workgroup order)
#include "common.h"

namespace {

using radmmm::lrelu;
using radmmm::ST;

// m = a > 0 ? gy : gy * slope ; q = m / div ; gx = accum ? gx + q : q  (the order the header states)
__device__ __forceinline__ float dlrelu(float gy, float a, float base, float div, float slope, int accum) {
  const float m = a > 0.f ? gy : gy * slope;
  const float q = m / div;
  return accum ? base + q : q;
}

// One float4 per thread over rows x cols/4.  gx carries no __restrict__: the generator calls this in place (gx == gy)
// and with accum, where every thread loads its float4s before it stores the same four floats.
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const float* gy, int ldgy, const float* a, int lda, float* gx,
                                                        int ldgx, long long rows, int cols, int T,
                                                        const int32_t* __restrict__ lens, float div, float slope,
                                                        int accum) {
  const int q = cols >> 2;
  const long long total = rows * q;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int c = (int)(i - r * q) * 4;
    const int b = (int)(r / T), t = (int)(r - (long long)b * T);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!lens || t < lens[b]) {
      const float4 g = *reinterpret_cast<const float4*>(gy + r * ldgy + c);
      const float4 s = *reinterpret_cast<const float4*>(a + r * lda + c);
      float4 base = o;
      if (accum) base = *reinterpret_cast<const float4*>(gx + r * ldgx + c);
      o.x = dlrelu(g.x, s.x, base.x, div, slope, accum);
      o.y = dlrelu(g.y, s.y, base.y, div, slope, accum);
      o.z = dlrelu(g.z, s.z, base.z, div, slope, accum);
      o.w = dlrelu(g.w, s.w, base.w, div, slope, accum);
    }
    *reinterpret_cast<float4*>(gx + r * ldgx + c) = o;
  }
}

// conv_post backward.  A workgroup of 256 threads owns chunks of `lanes * PB_ITERS` consecutive rows, lanes = 256 / (C/4):
// thread (lane, quad) keeps its four channels for the whole launch, so its taps x 4 weights and its taps x 4 partial
// weight gradients live in registers.  Per chunk the workgroup stages dpre = g (1 - audio^2) of the chunk's rows and the
// taps/2 rows on either side in LDS; a thread then reads one float4 of x per row, writes one float4 of dx and adds
// leaky_relu(x / div) dpre[r - (tap - taps/2)] to its partials: the same `taps` dpre values serve dx and dw.
constexpr int PB_TAPS = 7;
constexpr int PB_ITERS = 8;
constexpr int PB_MAX_BLOCKS = 1024;

inline int pb_chunk_rows(int C) { return (256 / (C >> 2)) * PB_ITERS; }
inline int pb_blocks(int rows, int C) {
  const long long chunks = ((long long)rows + pb_chunk_rows(C) - 1) / pb_chunk_rows(C);
  return (int)(chunks < PB_MAX_BLOCKS ? chunks : PB_MAX_BLOCKS);
}

__global__ __launch_bounds__(256) void conv_post_bwd_kernel(const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ w, int ldw,
                                                            const float* __restrict__ audio,
                                                            const float* __restrict__ g, float* __restrict__ dx,
                                                            int lddx, float* __restrict__ part, long long rows, int C,
                                                            int taps, int T, const int32_t* __restrict__ lens,
                                                            float div, float slope) {
  __shared__ float dp[256 * PB_ITERS + PB_TAPS - 1];
  __shared__ float red[256 * PB_TAPS * 4];
  __shared__ float redb[256];
  const int Q = C >> 2, lanes = 256 / Q, h = taps >> 1;
  const int tid = threadIdx.x, quad = tid % Q, lane = tid / Q;
  const bool active = lane < lanes;
  const int chunk_rows = lanes * PB_ITERS;
  const long long nchunks = (rows + chunk_rows - 1) / chunk_rows;
  float wr[PB_TAPS][4], acc[PB_TAPS][4], accb = 0.f;
#pragma unroll
  for (int tap = 0; tap < PB_TAPS; ++tap)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wr[tap][e] = (active && tap < taps) ? w[tap * ldw + quad * 4 + e] : 0.f;
      acc[tap][e] = 0.f;
    }
  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const long long r0 = chunk * chunk_rows;
    __syncthreads();
    for (int i = tid; i < chunk_rows + 2 * h; i += 256) {
      const long long r = r0 - h + i;
      float v = 0.f;
      if (r >= 0 && r < rows) {
        const int b = (int)(r / T), t = (int)(r - (long long)b * T);
        if (!lens || t < lens[b]) {
          const float a = audio[r];
          v = g[r] * (1.f - a * a);
        }
      }
      dp[i] = v;
    }
    __syncthreads();
    if (!active) continue;
    for (int it = 0; it < PB_ITERS; ++it) {
      const int lr = it * lanes + lane;
      const long long r = r0 + lr;
      if (r >= rows) break;
      const int b = (int)(r / T), t = (int)(r - (long long)b * T);
      const int len = lens ? lens[b] : T;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < len) {
        const float4 xv = *reinterpret_cast<const float4*>(x + r * ldx + quad * 4);
        const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
        float d[PB_TAPS];
#pragma unroll
        for (int tap = 0; tap < PB_TAPS; ++tap) {
          const int ts = t - (tap - h);
          d[tap] = (tap < taps && ts >= 0 && ts < len) ? dp[lr + 2 * h - tap] : 0.f;
        }
        float oe[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float s = 0.f;
          const float av = lrelu(xe[e] / div, slope);
#pragma unroll
          for (int tap = 0; tap < PB_TAPS; ++tap) {
            s = fmaf(wr[tap][e], d[tap], s);
            acc[tap][e] = fmaf(av, d[tap], acc[tap][e]);
          }
          oe[e] = (xe[e] > 0.f ? s : s * slope) / div;
        }
        o = make_float4(oe[0], oe[1], oe[2], oe[3]);
        if (quad == 0) accb += dp[lr + h];
      }
      *reinterpret_cast<float4*>(dx + r * lddx + quad * 4) = o;
    }
  }
  // the workgroup's partial row: the lanes' sums added in lane order
  __syncthreads();
#pragma unroll
  for (int tap = 0; tap < PB_TAPS; ++tap)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[tid * (PB_TAPS * 4) + tap * 4 + e] = acc[tap][e];
  redb[tid] = accb;
  __syncthreads();
  const long long psize = (long long)taps * ldw + 1;
  float* prow = part + blockIdx.x * psize;
  for (int j = tid; j < taps * C; j += 256) {
    const int tap = j / C, c = j - tap * C;
    float s = 0.f;
    for (int l = 0; l < lanes; ++l) s += red[(l * Q + (c >> 2)) * (PB_TAPS * 4) + tap * 4 + (c & 3)];
    prow[tap * ldw + c] = s;
  }
  if (tid == 0) {
    float s = 0.f;
    for (int l = 0; l < lanes; ++l) s += redb[l * Q];
    prow[(long long)taps * ldw] = s;
  }
}

// dw[tap*ldw + c] (0 for c >= C) and dbias[0]: the workgroups' partial rows added in workgroup order
__global__ __launch_bounds__(256) void conv_post_bwd_final_kernel(const float* __restrict__ part, int nparts,
                                                                  float* __restrict__ dw, float* __restrict__ dbias,
                                                                  int C, int taps, int ldw) {
  const int n = taps * ldw;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const long long psize = (long long)n + 1;
  const bool pad = i < n && (i % ldw) >= C;
  float s = 0.f;
  if (!pad)
    for (int p = 0; p < nparts; ++p) s += part[p * psize + i];
  if (i < n) dw[i] = s;
  else dbias[0] = s;
}

}  // namespace

extern "C" int32_t radmmm_voc_lrelu_bwd(const float* gy, int ldgy, const float* a, int lda, float* gx, int ldgx, int rows,
                                    int cols, int T, const int32_t* lens, float div, float slope, int accum,
                                    radmmm_stream_t stream) {
  RADMMM_REQUIRE(gy && a && gx, "voc_lrelu_bwd: null pointer");
  RADMMM_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0 && T > 0 && rows % T == 0 && ldgy % 4 == 0 && lda % 4 == 0 &&
                     ldgx % 4 == 0 && ldgy >= cols && lda >= cols && ldgx >= cols && div > 0.f,
                 "voc_lrelu_bwd: bad dims (rows=%d cols=%d T=%d ldgy=%d lda=%d ldgx=%d div=%g)", rows, cols, T, ldgy, lda,
                 ldgx, (double)div);
  RADMMM_REQUIRE(radmmm::aligned16(gy) && radmmm::aligned16(a) && radmmm::aligned16(gx),
                 "voc_lrelu_bwd: gy / a / gx must be 16B aligned");
  long long blocks = ((long long)rows * (cols / 4) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(lrelu_bwd_kernel, dim3((int)blocks), dim3(256), 0, ST(stream), gy, ldgy, a, lda, gx, ldgx,
                     (long long)rows, cols, T, lens, div, slope, accum);
  return radmmm::check_launch("voc_lrelu_bwd");
}

static bool pb_dims_ok(int rows, int C, int taps, int ldw) {
  return rows > 0 && C > 0 && C % 4 == 0 && C <= 1024 && taps >= 1 && taps % 2 == 1 && taps <= PB_TAPS && ldw >= C;
}

extern "C" int64_t radmmm_voc_conv_post_bwd_scratch_floats(int rows, int C, int taps, int ldw) {
  if (!pb_dims_ok(rows, C, taps, ldw)) return 0;
  return (int64_t)pb_blocks(rows, C) * ((int64_t)taps * ldw + 1);
}

extern "C" int32_t radmmm_voc_conv_post_bwd(const float* x, int ldx, const float* w, int ldw, const float* audio,
                                        const float* g, float* dx, int lddx, float* dw, float* dbias, float* scratch,
                                        int rows, int C, int taps, int T, const int32_t* lens, float div, float slope,
                                        radmmm_stream_t stream) {
  RADMMM_REQUIRE(x && w && audio && g && dx && dw && dbias && scratch, "voc_conv_post_bwd: null pointer");
  RADMMM_REQUIRE(pb_dims_ok(rows, C, taps, ldw) && T > 0 && rows % T == 0 && ldx % 4 == 0 && ldx >= C &&
                     lddx % 4 == 0 && lddx >= C && div > 0.f,
                 "voc_conv_post_bwd: bad dims (rows=%d C=%d taps=%d T=%d ldx=%d lddx=%d ldw=%d div=%g)", rows, C, taps, T,
                 ldx, lddx, ldw, (double)div);
  RADMMM_REQUIRE(radmmm::aligned16(x) && radmmm::aligned16(dx), "voc_conv_post_bwd: x / dx must be 16B aligned");
  const int nb = pb_blocks(rows, C);
  hipLaunchKernelGGL(conv_post_bwd_kernel, dim3(nb), dim3(256), 0, ST(stream), x, ldx, w, ldw, audio, g, dx, lddx,
                     scratch, (long long)rows, C, taps, T, lens, div, slope);
  int rc = radmmm::check_launch("voc_conv_post_bwd");
  if (rc) return rc;
  const int n = taps * ldw + 1;
  hipLaunchKernelGGL(conv_post_bwd_final_kernel, dim3((n + 255) / 256), dim3(256), 0, ST(stream), scratch, nb, dw,
                     dbias, C, taps, ldw);
  return radmmm::check_launch("voc_conv_post_bwd (final)");
}
