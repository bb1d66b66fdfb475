// Precision "h3" of the HiFi-GAN multi-period discriminator: the producers that hand the wide convs' three
// passes to the split-operand kernels (radmmm_rowgemm_h3, radmmm_wgrad_rm) in the pass that computes the value, so that no
// fp32 -> split pass of its own and no fp32 frame matrix exists in that mode.  Layouts are mpd.hip's: a padded map
// [S][H + 4][C], a dense matrix [S * H][C]; a pair is two half arrays (hi, lo) of scale * value, the bits of
// radmmm_split_f16 (split_pack.h store_split8_f16).
//
//   radmmm_mpdh3_repad            conv output -> leaky relu -> the fp32 padded map AND its padded pair (the framed A operand)
//   radmmm_mpdh3_frame            padded fp32 map -> the pair of its frame matrix [S * H'][5 * C] (the weight gradient's X)
//   radmmm_mpdh3_unframe          mpd_unframe with the pair of scale * dZ beside (or instead of) the fp32 dZ
//   radmmm_mpdh3_conv_post_dgrad  mpd_conv_post_dgrad in the same way
//   radmmm_mpdh3_plan             host only: can a conv run its three passes on the split kernels?
// The fp32 results repeat mpd.hip's arithmetic operation for operation (the same bits).  One thread owns 8 channels: two
// 16-byte fp32 accesses and one 16-byte store per half array.  Memory-bound, no LDS, no reductions; the one atomic is the
// saturation flag's OR.
#include "common.h"
#include "split_pack.h"

namespace {

using radmmm::grid_for;
using radmmm::lrelu;
using radmmm::ST;

__device__ __forceinline__ void load8(const float* __restrict__ p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ void store8(float* __restrict__ p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

__device__ __forceinline__ void zero_pair8(void* hi, void* lo, long long at) {
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  *reinterpret_cast<uint4*>(static_cast<_Float16*>(hi) + at) = z;
  *reinterpret_cast<uint4*>(static_cast<_Float16*>(lo) + at) = z;
}

// X[s][r][c] = 2 <= r < 2 + H ? lrelu(Z[(s * H + r - 2) * ldz + c]) : 0, and the pair of scale * X in the same layout
__global__ void __launch_bounds__(256) repad_h3_kernel(const float* __restrict__ Z, int ldz, float* __restrict__ X, void* Xh, void* Xl,
                                                       long long S, int H, int C, float slope, float scale, int32_t* sat_flag) {
  const int q = C >> 3, Hp = H + 4;
  const long long total = S * Hp * q;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 8;
    const long long sr = i / q;
    const int r = (int)(sr % Hp);
    const long long s = sr / Hp;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r >= 2 && r < 2 + H) {
      load8(Z + (s * H + r - 2) * ldz + c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = lrelu(v[e], slope);
      amax = fmaxf(amax, radmmm::store_split8_f16_amax(Xh, Xl, sr * C, c, scale, v));
    } else {
      zero_pair8(Xh, Xl, sr * C + c);
    }
    store8(X + sr * C + c, v);
  }
  radmmm::raise_sat_flag(sat_flag, amax);
}

// pair of F[(s * Ho + h') * ldf + j] = scale * X[(s * Hp + st * h') * C + j], j < 5C; zero rows from S * Ho on
__global__ void __launch_bounds__(256) frame_h3_kernel(const float* __restrict__ X, void* Fh, void* Fl, int ldf, long long rows,
                                                       long long rows_tot, int Hp, int C, int Ho, int st, float scale,
                                                       int32_t* sat_flag) {
  const int q = 5 * C / 8;
  const long long total = rows_tot * q;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i % q) * 8;
    const long long row = i / q;
    if (row >= rows) {
      zero_pair8(Fh, Fl, row * ldf + j);
      continue;
    }
    const int h1 = (int)(row % Ho);
    const long long s = row / Ho;
    float v[8];
    load8(X + (s * Hp + (long long)st * h1) * C + j, v);
    amax = fmaxf(amax, radmmm::store_split8_f16_amax(Fh, Fl, row * ldf, j, scale, v));
  }
  radmmm::raise_sat_flag(sat_flag, amax);
}

// times the leaky-relu derivative from the saved map, then dZ (optional) and the pair of scale * dZ
__device__ __forceinline__ float finish_dz(float (&g)[8], const float* __restrict__ add, const float* __restrict__ X, long long at,
                                           float slope, float* __restrict__ dZ, void* dZh, void* dZl, int ldh, long long row, int c,
                                           int C, float scale) {
  if (add) {
    float t[8];
    load8(add + at, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] += t[e];
  }
  float x[8];
  load8(X + at, x);
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] *= x[e] > 0.f ? 1.f : slope;
  if (dZ) store8(dZ + row * C + c, g);
  return radmmm::store_split8_f16_amax(dZh, dZl, row * ldh, c, scale, g);
}

// mpd.hip unframe_kernel's sum, 8 channels per thread; rows from S * H on of the pair are zeros
__global__ void __launch_bounds__(256) unframe_h3_kernel(const float* __restrict__ dF, const float* __restrict__ add,
                                                         const float* __restrict__ X, float* __restrict__ dZ, void* dZh, void* dZl,
                                                         int ldh, long long rows, long long rows_tot, int H, int C, int Ho, int st,
                                                         float slope, float scale, int32_t* sat_flag) {
  const int q = C >> 3, Hp = H + 4;
  const long long total = rows_tot * q;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 8;
    const long long row = i / q;
    if (row >= rows) {
      zero_pair8(dZh, dZl, row * ldh + c);
      continue;
    }
    const int h = (int)(row % H);
    const long long s = row / H;
    const int u = h + 2;
    int lo = u - 4 > 0 ? (u - 4 + st - 1) / st : 0;
    int hi = u / st;
    if (hi > Ho - 1) hi = Ho - 1;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int h1 = lo; h1 <= hi; ++h1) {
      float t[8];
      load8(dF + ((s * Ho + h1) * 5 + (u - st * h1)) * C + c, t);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += t[e];
    }
    amax = fmaxf(amax, finish_dz(g, add, X, (s * Hp + u) * C + c, slope, dZ, dZh, dZl, ldh, row, c, C, scale));
  }
  radmmm::raise_sat_flag(sat_flag, amax);
}

// mpd.hip conv_post_dgrad_kernel's sum, 8 channels per thread
__global__ void __launch_bounds__(256) conv_post_dgrad_h3_kernel(const float* __restrict__ dOut, const float* __restrict__ W,
                                                                 const float* __restrict__ add, const float* __restrict__ X,
                                                                 float* __restrict__ dZ, void* dZh, void* dZl, int ldh, long long rows,
                                                                 long long rows_tot, int p, int H, int C, float slope, float scale,
                                                                 int32_t* sat_flag) {
  const int q = C >> 3, Hp = H + 4;
  const long long total = rows_tot * q;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 8;
    const long long row = i / q;
    if (row >= rows) {
      zero_pair8(dZh, dZl, row * ldh + c);
      continue;
    }
    const int h = (int)(row % H);
    const long long s = row / H;
    const int w = (int)(s % p);
    const float* go = dOut + (s / p) * H * p + w;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) {
      const int ho = h + 1 - k;
      if (ho < 0 || ho >= H) continue;
      const float d = go[(long long)ho * p];
      float t[8];
      load8(W + k * C + c, t);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += d * t[e];
    }
    amax = fmaxf(amax, finish_dz(g, add, X, (s * Hp + 2 + h) * C + c, slope, dZ, dZh, dZl, ldh, row, c, C, scale));
  }
  radmmm::raise_sat_flag(sat_flag, amax);
}

int check_map8(const char* who, int S, int H, int C) {
  RADMMM_REQUIRE(S > 0 && H > 0 && C > 0 && C % 8 == 0, "%s: bad dims (S=%d H=%d C=%d; C must be a multiple of 8)", who, S, H, C);
  RADMMM_REQUIRE((long long)S * (H + 4) * C * 4 < 0x7fffffffLL, "%s: the map exceeds 2 GiB", who);
  return 0;
}

// a pair of max(rows, rows_pad) rows of `cols` columns at pitch ld
int check_pair(const char* who, const void* hi, const void* lo, int ld, long long rows, int rows_pad, int cols, float scale) {
  RADMMM_REQUIRE(hi && lo && radmmm::aligned16(hi) && radmmm::aligned16(lo), "%s: the pair must be two 16-byte aligned arrays", who);
  RADMMM_REQUIRE(ld % 8 == 0 && ld >= cols && rows_pad >= 0, "%s: pair pitch %d (%% 8 == 0, >= %d columns), rows_pad %d", who, ld, cols, rows_pad);
  RADMMM_REQUIRE((rows > rows_pad ? rows : rows_pad) * ld * 2 < 0x7fffffffLL, "%s: the pair exceeds 2 GiB", who);
  RADMMM_REQUIRE(scale > 0.f && scale <= 3.4e38f, "%s: scale must be positive and finite", who);
  return 0;
}

int check_windows(const char* who, int H, int Ho, int stride) {
  RADMMM_REQUIRE(stride >= 1 && Ho >= 1 && (long long)stride * (Ho - 1) + 5 <= H + 4, "%s: %d windows of stride %d leave the %d + 4 rows", who,
                 Ho, stride, H);
  return 0;
}

}  // namespace

extern "C" int radmmm_mpdh3_repad(const float* Z, int ldz, float* X, void* Xh, void* Xl, int S, int H, int C, float slope, float scale,
                                   int32_t* sat_flag, radmmm_stream_t stream) {
  RADMMM_REQUIRE(Z && X, "mpdh3_repad: null pointer");
  if (int rc = check_map8("mpdh3_repad", S, H, C)) return rc;
  if (int rc = check_pair("mpdh3_repad", Xh, Xl, C, (long long)S * (H + 4), 0, C, scale)) return rc;
  RADMMM_REQUIRE(ldz % 4 == 0 && ldz >= C && radmmm::aligned16(Z) && radmmm::aligned16(X), "mpdh3_repad: 16B alignment (ldz=%d)", ldz);
  RADMMM_REQUIRE((long long)S * H * ldz * 4 < 0x7fffffffLL, "mpdh3_repad: Z exceeds 2 GiB");
  hipLaunchKernelGGL(repad_h3_kernel, dim3(grid_for((long long)S * (H + 4) * (C / 8), 256)), dim3(256), 0, ST(stream), Z, ldz, X, Xh,
                     Xl, (long long)S, H, C, slope, scale, sat_flag);
  return radmmm::check_launch("mpdh3_repad");
}

extern "C" int radmmm_mpdh3_frame(const float* X, void* Fh, void* Fl, int ldf, int S, int H, int C, int Ho, int stride, int rows_pad,
                                   float scale, int32_t* sat_flag, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && radmmm::aligned16(X), "mpdh3_frame: X null or not 16-byte aligned");
  if (int rc = check_map8("mpdh3_frame", S, H, C)) return rc;
  if (int rc = check_windows("mpdh3_frame", H, Ho, stride)) return rc;
  const long long rows = (long long)S * Ho;
  if (int rc = check_pair("mpdh3_frame", Fh, Fl, ldf, rows, rows_pad, 5 * C, scale)) return rc;
  const long long rows_tot = rows > rows_pad ? rows : rows_pad;
  hipLaunchKernelGGL(frame_h3_kernel, dim3(grid_for(rows_tot * (5 * C / 8), 256)), dim3(256), 0, ST(stream), X, Fh, Fl, ldf, rows,
                     rows_tot, H + 4, C, Ho, stride, scale, sat_flag);
  return radmmm::check_launch("mpdh3_frame");
}

extern "C" int radmmm_mpdh3_unframe(const float* dF, const float* add, const float* X, float* dZ, void* dZh, void* dZl, int ldh, int S,
                                     int H, int C, int Ho, int stride, float slope, int rows_pad, float scale, int32_t* sat_flag,
                                     radmmm_stream_t stream) {
  RADMMM_REQUIRE(dF && X, "mpdh3_unframe: null pointer");
  if (int rc = check_map8("mpdh3_unframe", S, H, C)) return rc;
  if (int rc = check_windows("mpdh3_unframe", H, Ho, stride)) return rc;
  RADMMM_REQUIRE((long long)S * Ho * 5 * C * 4 < 0x7fffffffLL, "mpdh3_unframe: the frame matrix exceeds 2 GiB");
  const long long rows = (long long)S * H;
  if (int rc = check_pair("mpdh3_unframe", dZh, dZl, ldh, rows, rows_pad, C, scale)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(dF) && radmmm::aligned16(X) && radmmm::aligned16(dZ) && radmmm::aligned16(add),
                 "mpdh3_unframe: 16B alignment");
  const long long rows_tot = rows > rows_pad ? rows : rows_pad;
  hipLaunchKernelGGL(unframe_h3_kernel, dim3(grid_for(rows_tot * (C / 8), 256)), dim3(256), 0, ST(stream), dF, add, X, dZ, dZh, dZl,
                     ldh, rows, rows_tot, H, C, Ho, stride, slope, scale, sat_flag);
  return radmmm::check_launch("mpdh3_unframe");
}

extern "C" int radmmm_mpdh3_conv_post_dgrad(const float* dOut, const float* W, const float* add, const float* X, float* dZ, void* dZh,
                                             void* dZl, int ldh, int B2, int p, int H, int C, float slope, int rows_pad, float scale,
                                             int32_t* sat_flag, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dOut && W && X, "mpdh3_conv_post_dgrad: null pointer");
  RADMMM_REQUIRE(B2 > 0 && p > 0 && (long long)B2 * p < 0x7fffffffLL, "mpdh3_conv_post_dgrad: bad dims (B2=%d p=%d)", B2, p);
  if (int rc = check_map8("mpdh3_conv_post_dgrad", B2 * p, H, C)) return rc;
  const long long rows = (long long)B2 * p * H;
  if (int rc = check_pair("mpdh3_conv_post_dgrad", dZh, dZl, ldh, rows, rows_pad, C, scale)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(W) && radmmm::aligned16(X) && radmmm::aligned16(dZ) && radmmm::aligned16(add),
                 "mpdh3_conv_post_dgrad: 16B alignment");
  const long long rows_tot = rows > rows_pad ? rows : rows_pad;
  hipLaunchKernelGGL(conv_post_dgrad_h3_kernel, dim3(grid_for(rows_tot * (C / 8), 256)), dim3(256), 0, ST(stream), dOut, W, add, X, dZ,
                     dZh, dZl, ldh, rows, rows_tot, p, H, C, slope, scale, sat_flag);
  return radmmm::check_launch("mpdh3_conv_post_dgrad");
}

// The decision the discriminator's precision plan reports and its launches follow.  The two GEMM descriptors are the ones
// rad_mmm_amd/discriminators.py builds (any aligned address stands for an operand: the plan looks at presence and
// alignment only); the weight gradient's conditions are radmmm_wgrad_rm's at one tap.
extern "C" int radmmm_mpdh3_plan(int S, int Hin, int Cin, int Hout, int Cout, int stride) {
  RADMMM_REQUIRE(S > 0 && Hin > 0 && Cin > 0 && Hout > 0 && Cout > 0, "mpdh3_plan: bad dims (S=%d Hin=%d Cin=%d Hout=%d Cout=%d)", S, Hin,
                 Cin, Hout, Cout);
  if (int rc = check_windows("mpdh3_plan", Hin, Hout, stride)) return rc;
  if (Cin % 8 || Cout % 8) {
    radmmm::set_error("mpdh3_plan: the pair producers need channels %% 8 == 0 (%d -> %d)", Cin, Cout);
    return 0;
  }
  const long long R = (long long)S * Hout, Rp = R > 32 ? R : 32;
  if ((long long)S * (Hin + 4) * Cin * 4 >= 0x7fffffffLL || R * 5 * Cin * 4 >= 0x7fffffffLL || Rp * 5 * Cin * 2 >= 0x7fffffffLL ||
      Rp * Cout * 4 >= 0x7fffffffLL) {
    radmmm::set_error("mpdh3_plan: an operand of %lld rows exceeds 2 GiB", R);
    return 0;
  }
  void* const any = reinterpret_cast<void*>(uintptr_t(256));
  radmmm::h3_plan pl;
  radmmm_rowgemm_h3_desc f = {};
  f.base.sign = 1; f.base.taps = 1; f.base.dil = 1; f.base.ratio_taps = 1; f.base.ratio_dil = 1;
  f.Ah = f.Al = f.Bh = f.Bl = any; f.base.C = static_cast<float*>(any); f.acc_scale = 1.f; f.nprod = 3;
  radmmm_rowgemm_h3_desc g = f;
  f.base.a_item_stride = (int64_t)(Hin + 4) * Cin; f.lda_h = stride * Cin; f.ldb_h = 5 * Cin; f.base.bias = static_cast<float*>(any);
  f.base.ldc = Cout; f.base.M = (int)R; f.base.N = Cout; f.base.K = 5 * Cin; f.base.T = Hout;
  if (radmmm::plan_rowgemm_h3(&f, &pl)) return 0;                   // (the reason is the planner's text)
  g.lda_h = Cout; g.ldb_h = Cout; g.base.ldc = 5 * Cin; g.base.M = (int)R; g.base.N = 5 * Cin; g.base.K = Cout; g.base.T = Hout;
  if (radmmm::plan_rowgemm_h3(&g, &pl)) return 0;
  // radmmm_wgrad_rm(GY = the dZ pair [Rp][Cout], X = the frame pair [Rp][5 Cin], R = T = Rp, one tap): pitches % 8 hold with
  // the channels', T >= 32 and one utterance by construction, the extents were checked above
  return 1;
}
