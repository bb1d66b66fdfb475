// Grouped strided 1-d convolution on the fp32 matrix cores of gfx950: forward, data gradient and weight gradient.  The kernel
// family of the HiFi-GAN multi-scale discriminator's hot path (hifigan_models.py: DiscriminatorS, five grouped, strided,
// 41-tap Conv1d layers), which neither the taps mode nor the framed form of radmmm_rowgemm_f32 can express.
//
// Layout.  A feature map is a channels-last PADDED buffer [S][pad + H + pad][C]: S sequences, pad zero rows on either side
// of every sequence, pad = k / 2 of the conv that READS the map.  With G groups, C_in = G * Cin_g and C_out = G * Cout_g;
// window h' of group g is rows st * h' .. st * h' + k - 1, columns g * Cin_g .. (g + 1) * Cin_g of the padded input.  The
// weight is packed [G][Cout_g][k * Cin_g], kk = tap * Cin_g + ci.  A DENSE matrix is [S * H][C].
//
//   radmmm_msd_gconv_fwd     Y[s][po + h'][g Cout_g + co] = lrelu(bias + sum_kk X[s][st h' + tap][g Cin_g + ci] * W[g][co][kk]),
//                            written straight into the next conv's padded buffer, its 2 * po pad rows as zeros.  No frame
//                            matrix: a tile's st * 31 + k input rows are staged in LDS once for all taps.
//   radmmm_msd_gconv_dgrad   the adjoint in gather form: an input row sums, windows ascending, the windows that hold it (the taps
//                            congruent to its phase modulo the stride), adds the map's own gradient and multiplies by the
//                            leaky-relu derivative taken from the saved map.
//   radmmm_msd_gconv_wgrad   P[split][g][co][kk] = sum over the split's (s, h') of dZ[s][h'][g Cout_g + co] * X[s][st h' + tap][..];
//                            fixed split ranges, radmmm_colsum_final adds them.
// Every contraction is a chain of v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulate) in a fixed order; no atomics.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

using radmmm::grid_for;
using radmmm::lrelu;
using radmmm::ST;

constexpr int kRows = 32;        // output rows (fwd), input rows of one phase (dgrad), contraction rows per step (wgrad)
constexpr int kChunk = 64;       // weight columns kk staged per step of the forward
constexpr int kSlack = 64;       // floats past either LDS array: a masked MFMA column may read (never use) them
constexpr int kWgradTaps = 4;    // taps per workgroup of the weight gradient: one per wave
constexpr int kMaxSplits = 64;

struct GconvArgs {
  int S, Hin, Hout, G, Cin_g, Cout_g, k, st, pad_out;
  float slope;
};

// Xs [st * 31 + k][Cin_g + 4]: the tile's input rows; Ws [64][kChunk + 4]: W[g][co][kk0 .. kk0 + 64).  Wave w owns the
// 16 x 16 subtiles j = w, w + 4 of the 2 x ceil(Cout_g / 16) grid: row half j & 1, column block j >> 1.
__global__ void __launch_bounds__(256) gconv_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ Y, GconvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.y, s = blockIdx.z, h0 = blockIdx.x * kRows;
  const int Cin = a.G * a.Cin_g, Cout = a.G * a.Cout_g, Hp = a.Hin + a.k - 1, Hpo = a.Hout + 2 * a.pad_out;
  const int K = a.k * a.Cin_g, PA = a.Cin_g + 4, PW = kChunk + 4, rin = a.st * (kRows - 1) + a.k;
  float* Xs = smem;
  float* Ws = smem + rin * PA + kSlack;

  if (blockIdx.x == 0) {   // the output's pad rows of this group's columns
    const int q = a.Cout_g >> 2;
    for (int i = tid; i < 2 * a.pad_out * q; i += 256) {
      const int c = (i % q) * 4, r = i / q;
      const int row = r < a.pad_out ? r : a.Hout + r;
      *reinterpret_cast<float4*>(Y + ((long long)s * Hpo + row) * Cout + g * a.Cout_g + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  {
    const int q = a.Cin_g >> 2;
    const float* src = X + (long long)s * Hp * Cin + g * a.Cin_g;
    for (int i = tid; i < rin * q; i += 256) {
      const int c = (i % q) * 4, r = i / q;
      const int pr = a.st * h0 + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pr < Hp) v = *reinterpret_cast<const float4*>(src + (long long)pr * Cin + c);
      *reinterpret_cast<float4*>(Xs + r * PA + c) = v;
    }
  }
  const int nsub = 2 * ((a.Cout_g + 15) >> 4);
  const int rt = wave & 1;
  const int ct0 = wave >> 1, ct1 = (wave + 4) >> 1;
  const bool on0 = wave < nsub, on1 = wave + 4 < nsub;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const float* wsrc = W + (long long)g * a.Cout_g * K;
  const int arow = a.st * (rt * 16 + (lane & 15));
  for (int kk0 = 0; kk0 < K; kk0 += kChunk) {
    const int kc = K - kk0 < kChunk ? K - kk0 : kChunk;
    __syncthreads();
    for (int i = tid; i < a.Cout_g * (kChunk / 4); i += 256) {
      const int c = (i & (kChunk / 4 - 1)) * 4, co = i / (kChunk / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < kc) v = *reinterpret_cast<const float4*>(wsrc + (long long)co * K + kk0 + c);
      *reinterpret_cast<float4*>(Ws + co * PW + c) = v;
    }
    __syncthreads();
    if (on0) {
      for (int c = 0; c < kc; c += 4) {
        const int kk = kk0 + c;
        const int tap = kk / a.Cin_g, ci = kk - tap * a.Cin_g;
        const float av = Xs[(arow + tap) * PA + ci + (lane >> 4)];
        const float b0 = Ws[(ct0 * 16 + (lane & 15)) * PW + c + (lane >> 4)];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
        if (on1) {
          const float b1 = Ws[(ct1 * 16 + (lane & 15)) * PW + c + (lane >> 4)];
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
        }
      }
    }
  }
  // C/D layout of 16x16x4: lane l, register e -> column l & 15, row 4 (l >> 4) + e
#pragma unroll
  for (int slot = 0; slot < 2; ++slot) {
    const bool on = slot ? on1 : on0;
    const int co = (slot ? ct1 : ct0) * 16 + (lane & 15);
    if (!on || co >= a.Cout_g) continue;
    const float bv = bias[g * a.Cout_g + co];
    const f32x4 acc = slot ? acc1 : acc0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int h = h0 + rt * 16 + 4 * (lane >> 4) + e;
      if (h < a.Hout) Y[((long long)s * Hpo + a.pad_out + h) * Cout + g * a.Cout_g + co] = lrelu(acc[e] + bv, a.slope);
    }
  }
}

// One workgroup: 32 padded input rows u = st * m + ph of one phase ph, one group, one sequence.  The taps of that phase are
// st * j + ph, j < J, and row u lies in window h' = m - j: a stride-1 correlation of dY along m.  dYs [31 + J][Cout_g + 4]
// holds windows m0 - (J - 1) .. m0 + 31; Ws [Cout_g][tc * Cin_g + 4] the weights of tc taps at a time.  Windows ascending =
// j descending.  Wave w owns the subtiles j = w, w + 4 of the 2 x ceil(Cin_g / 16) grid.
__global__ void __launch_bounds__(256) gconv_dgrad_kernel(const float* __restrict__ dY, const float* __restrict__ W,
                                                          const float* __restrict__ add, const float* __restrict__ X,
                                                          float* __restrict__ dX, GconvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.y, s = blockIdx.z;
  const int ph = blockIdx.x % a.st, m0 = (blockIdx.x / a.st) * kRows;
  const int Cin = a.G * a.Cin_g, Cout = a.G * a.Cout_g, pin = a.k >> 1, Hp = a.Hin + a.k - 1;
  const int K = a.k * a.Cin_g;
  const int J = ph < a.k ? (a.k - 1 - ph) / a.st + 1 : 0;
  const int jmax = (a.k - 1) / a.st + 1;                       // the LDS carve-up does not depend on the phase
  const int tc = a.Cin_g >= kChunk ? 1 : kChunk / a.Cin_g;     // taps per stage
  const int PZ = a.Cout_g + 4, PW = tc * a.Cin_g + 4;
  float* Zs = smem;
  float* Ws = smem + (kRows - 1 + jmax) * PZ + kSlack;

  {
    const int q = a.Cout_g >> 2;
    const float* src = dY + (long long)s * a.Hout * Cout + g * a.Cout_g;
    for (int i = tid; i < (kRows - 1 + J) * q; i += 256) {
      const int c = (i % q) * 4, r = i / q;
      const int hw = m0 - (J - 1) + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (hw >= 0 && hw < a.Hout) v = *reinterpret_cast<const float4*>(src + (long long)hw * Cout + c);
      *reinterpret_cast<float4*>(Zs + r * PZ + c) = v;
    }
  }
  const int nsub = 2 * ((a.Cin_g + 15) >> 4);
  const int rt = wave & 1;
  const int ct0 = wave >> 1, ct1 = (wave + 4) >> 1;
  const bool on0 = wave < nsub, on1 = wave + 4 < nsub;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const float* wsrc = W + (long long)g * a.Cout_g * K;
  const int arow = rt * 16 + (lane & 15);
  for (int jj0 = 0; jj0 < J; jj0 += tc) {        // jj = J - 1 - j ascending: window m - j = m - (J - 1) + jj ascending
    const int nt = J - jj0 < tc ? J - jj0 : tc;
    __syncthreads();
    const int q = a.Cin_g >> 2;
    for (int i = tid; i < a.Cout_g * nt * q; i += 256) {
      const int c = (i % q) * 4;
      const int t = (i / q) % nt, co = i / (q * nt);
      const int tap = a.st * (J - 1 - (jj0 + t)) + ph;
      *reinterpret_cast<float4*>(Ws + co * PW + t * a.Cin_g + c) =
          *reinterpret_cast<const float4*>(wsrc + (long long)co * K + tap * a.Cin_g + c);
    }
    __syncthreads();
    if (on0) {
      for (int t = 0; t < nt; ++t) {
        const float* zr = Zs + (arow + jj0 + t) * PZ + (lane >> 4);
        const float* wr = Ws + (lane >> 4) * PW + t * a.Cin_g + (lane & 15);
        for (int c = 0; c < a.Cout_g; c += 4) {
          const float av = zr[c];
          const float b0 = wr[c * PW + ct0 * 16];
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
          if (on1) {
            const float b1 = wr[c * PW + ct1 * 16];
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
          }
        }
      }
    }
  }
#pragma unroll
  for (int slot = 0; slot < 2; ++slot) {
    const bool on = slot ? on1 : on0;
    const int ci = (slot ? ct1 : ct0) * 16 + (lane & 15);
    if (!on || ci >= a.Cin_g) continue;
    const f32x4 acc = slot ? acc1 : acc0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + rt * 16 + 4 * (lane >> 4) + e;
      const int u = a.st * m + ph, h = u - pin;
      if (h < 0 || h >= a.Hin) continue;
      const long long at = ((long long)s * Hp + u) * Cin + g * a.Cin_g + ci;
      float v = acc[e];
      if (add) v += add[at];
      v *= X[at] > 0.f ? 1.f : a.slope;
      dX[((long long)s * a.Hin + h) * Cin + g * a.Cin_g + ci] = v;
    }
  }
}

// One workgroup: split blockIdx.z, group blockIdx.y, taps 4 blockIdx.x + wave.  A unit is 32 windows of one sequence;
// the split walks its fixed range of units in order.  Per unit Zs [32][Cout_g + 4] holds dZ and Xs [st * 31 + 4][Cin_g + 4]
// the input rows the four taps reach; a wave keeps the whole [Cout_g][Cin_g] block of its tap in accumulators.
__global__ void __launch_bounds__(256) gconv_wgrad_kernel(const float* __restrict__ dZ, const float* __restrict__ X,
                                                          float* __restrict__ P, GconvArgs a, int nsplit) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tap0 = blockIdx.x * kWgradTaps, g = blockIdx.y, sp = blockIdx.z;
  const int Cin = a.G * a.Cin_g, Cout = a.G * a.Cout_g, Hp = a.Hin + a.k - 1, K = a.k * a.Cin_g;
  const int PZ = a.Cout_g + 4, PX = a.Cin_g + 4, rin = a.st * (kRows - 1) + kWgradTaps;
  float* Zs = smem;
  float* Xs = smem + kRows * PZ + kSlack;
  const int nch = (a.Hout + kRows - 1) / kRows;
  const long long units = (long long)a.S * nch;
  const int u_lo = (int)(units * sp / nsplit), u_hi = (int)(units * (sp + 1) / nsplit);
  const int no = (a.Cout_g + 15) >> 4, ni = (a.Cin_g + 15) >> 4;
  const bool on = tap0 + wave < a.k;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int u = u_lo; u < u_hi; ++u) {
    const int s = u / nch, h0 = (u - s * nch) * kRows;
    __syncthreads();
    {
      const int q = a.Cout_g >> 2;
      const float* src = dZ + (long long)s * a.Hout * Cout + g * a.Cout_g;
      for (int i = tid; i < kRows * q; i += 256) {
        const int c = (i % q) * 4, r = i / q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (h0 + r < a.Hout) v = *reinterpret_cast<const float4*>(src + (long long)(h0 + r) * Cout + c);
        *reinterpret_cast<float4*>(Zs + r * PZ + c) = v;
      }
    }
    {
      const int q = a.Cin_g >> 2;
      const float* src = X + (long long)s * Hp * Cin + g * a.Cin_g;
      for (int i = tid; i < rin * q; i += 256) {
        const int c = (i % q) * 4, r = i / q;
        const int pr = a.st * h0 + tap0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pr < Hp) v = *reinterpret_cast<const float4*>(src + (long long)pr * Cin + c);
        *reinterpret_cast<float4*>(Xs + r * PX + c) = v;
      }
    }
    __syncthreads();
    if (on) {
      for (int r0 = 0; r0 < kRows; r0 += 4) {
        const int r = r0 + (lane >> 4);
        const float* zr = Zs + r * PZ + (lane & 15);
        const float* xr = Xs + (a.st * r + wave) * PX + (lane & 15);
        float bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = j < ni ? xr[j * 16] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i < no) {
            const float av = zr[i * 16];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < ni) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  }
  if (!on) return;
  float* out = P + ((long long)sp * a.G + g) * a.Cout_g * K + (long long)(tap0 + wave) * a.Cin_g;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ci = j * 16 + (lane & 15);
      if (i >= no || j >= ni || ci >= a.Cin_g) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = i * 16 + 4 * (lane >> 4) + e;
        if (co < a.Cout_g) out[(long long)co * K + ci] = acc[i][j][e];
      }
    }
}

// out[(sig * B + b) * To + j] = (x[2j - 2] + x[2j - 1] + x[2j] + x[2j + 1]) / 4, x = 0 outside [0, T)
__global__ void __launch_bounds__(256) avgpool_kernel(const float* __restrict__ y, const float* __restrict__ yh, int ldy,
                                                      float* __restrict__ out, int B, int T, int To) {
  const long long total = 2LL * B * To;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i % To);
    const int sb = (int)(i / To);
    const int sig = sb / B, b = sb - sig * B;
    const float* x = (sig ? yh : y) + (long long)b * ldy;
    float acc = 0.f;
    for (int t = 2 * j - 2; t <= 2 * j + 1; ++t)
      if (t >= 0 && t < T) acc += x[t];
    out[i] = 0.25f * acc;
  }
}

// gx[n][t] = (sum of g[n][j] over the windows j (ascending) with 2j - 2 <= t <= 2j + 1, j < To) / 4
__global__ void __launch_bounds__(256) avgpool_bwd_kernel(const float* __restrict__ g, float* __restrict__ gx, int ldx, long long N,
                                                          int T, int To) {
  const long long total = N * T;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const long long n = i / T;
    const int lo = t >> 1;                 // ceil((t - 1) / 2)
    float acc = g[n * To + lo];            // lo <= (T - 1) / 2 < To
    if (lo + 1 < To) acc += g[n * To + lo + 1];
    gx[n * ldx + t] = 0.25f * acc;
  }
}

// F[(s * T + t) * 16 + j] = x_s[t - 7 + j] for j < 15 (0 outside [0, T)), 0 for j = 15; s = sig * B + b
__global__ void __launch_bounds__(256) frame15_kernel(const float* __restrict__ y, const float* __restrict__ yh, int ldy,
                                                      float* __restrict__ F, int B, int T) {
  const long long total = 2LL * B * T * 16;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i & 15);
    const long long row = i >> 4;
    const int t = (int)(row % T);
    const int sb = (int)(row / T);
    const int sig = sb / B, b = sb - sig * B;
    const int u = t - 7 + j;
    F[i] = (j < 15 && u >= 0 && u < T) ? (sig ? yh : y)[(long long)b * ldy + u] : 0.f;
  }
}

// g[n][u] = sum over the windows t = u + 7 - j (ascending: j from 14 down), 0 <= t < T, of dF[(n * T + t) * 16 + j]
__global__ void __launch_bounds__(256) unframe15_kernel(const float* __restrict__ dF, float* __restrict__ g, int ldg, long long N,
                                                        int T) {
  const long long total = N * T;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int u = (int)(i % T);
    const long long n = i / T;
    float acc = 0.f;
    for (int j = 14; j >= 0; --j) {
      const int t = u + 7 - j;
      if (t >= 0 && t < T) acc += dF[(n * T + t) * 16 + j];
    }
    g[n * ldg + u] = acc;
  }
}

// X[s][r][c] = pad <= r < pad + H ? lrelu(Z[(s * H + r - pad) * ldz + c]) : 0
__global__ void __launch_bounds__(256) repad_kernel(const float* __restrict__ Z, int ldz, float* __restrict__ X, long long S, int H,
                                                    int C, int pad, float slope) {
  const int q = C >> 2, Hp = H + 2 * pad;
  const long long total = S * Hp * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 4;
    const long long sr = i / q;
    const int r = (int)(sr % Hp);
    const long long s = sr / Hp;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= pad && r < pad + H) {
      v = *reinterpret_cast<const float4*>(Z + (s * H + r - pad) * ldz + c);
      v.x = lrelu(v.x, slope);
      v.y = lrelu(v.y, slope);
      v.z = lrelu(v.z, slope);
      v.w = lrelu(v.w, slope);
    }
    *reinterpret_cast<float4*>(X + sr * C + c) = v;
  }
}

int check_gconv(const char* who, int S, int Hin, int Hout, int G, int Cin_g, int Cout_g, int k, int stride, GconvArgs* a) {
  RADMMM_REQUIRE(k >= 1 && k <= 41 && (k & 1), "%s: k must be odd and at most 41 (k=%d)", who, k);
  RADMMM_REQUIRE(stride == 1 || stride == 2 || stride == 4, "%s: stride must be 1, 2 or 4 (stride=%d)", who, stride);
  RADMMM_REQUIRE(Cin_g >= 4 && Cin_g <= 64 && Cin_g % 4 == 0 && Cout_g >= 4 && Cout_g <= 64 && Cout_g % 4 == 0,
                 "%s: Cin_g and Cout_g must be multiples of 4 in [4, 64] (Cin_g=%d Cout_g=%d)", who, Cin_g, Cout_g);
  RADMMM_REQUIRE(S > 0 && S <= 65535 && G > 0 && G <= 65535 && Hin > 0, "%s: bad dims (S=%d G=%d Hin=%d)", who, S, G, Hin);
  RADMMM_REQUIRE(Hout == (Hin - 1) / stride + 1, "%s: Hout=%d does not belong to Hin=%d, stride %d (pad k / 2)", who, Hout, Hin, stride);
  const long long big = (long long)G * (Cin_g > Cout_g ? Cin_g : Cout_g);
  RADMMM_REQUIRE((long long)S * (Hin + k - 1) * big * 4 < 0x7fffffffLL, "%s: a map exceeds 2 GiB", who);
  a->S = S; a->Hin = Hin; a->Hout = Hout; a->G = G; a->Cin_g = Cin_g; a->Cout_g = Cout_g; a->k = k; a->st = stride;
  a->pad_out = 0; a->slope = 1.f;
  return 0;
}

}  // namespace

extern "C" int radmmm_msd_gconv_fwd(const float* X, const float* W, const float* bias, float* Y, int S, int Hin, int Hout, int G,
                                    int Cin_g, int Cout_g, int k, int stride, int pad_out, float slope, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && W && bias && Y, "msd_gconv_fwd: null pointer");
  GconvArgs a;
  if (int rc = check_gconv("msd_gconv_fwd", S, Hin, Hout, G, Cin_g, Cout_g, k, stride, &a)) return rc;
  RADMMM_REQUIRE(pad_out >= 0 && pad_out <= 20, "msd_gconv_fwd: pad_out must lie in [0, 20] (pad_out=%d)", pad_out);
  RADMMM_REQUIRE((long long)S * (Hout + 2 * pad_out) * G * Cout_g * 4 < 0x7fffffffLL, "msd_gconv_fwd: the output map exceeds 2 GiB");
  RADMMM_REQUIRE(radmmm::aligned16(X) && radmmm::aligned16(W) && radmmm::aligned16(Y), "msd_gconv_fwd: 16B alignment");
  a.pad_out = pad_out;
  a.slope = slope;
  const int rin = stride * (kRows - 1) + k;
  const size_t lds = (size_t)(rin * (Cin_g + 4) + kSlack + 64 * (kChunk + 4) + kSlack) * sizeof(float);
  hipLaunchKernelGGL(gconv_fwd_kernel, dim3((Hout + kRows - 1) / kRows, G, S), dim3(256), lds, ST(stream), X, W, bias, Y, a);
  return radmmm::check_launch("msd_gconv_fwd");
}

extern "C" int radmmm_msd_gconv_dgrad(const float* dY, const float* W, const float* add, const float* X, float* dX, int S, int Hin,
                                      int Hout, int G, int Cin_g, int Cout_g, int k, int stride, float slope,
                                      radmmm_stream_t stream) {
  RADMMM_REQUIRE(dY && W && X && dX, "msd_gconv_dgrad: null pointer");
  GconvArgs a;
  if (int rc = check_gconv("msd_gconv_dgrad", S, Hin, Hout, G, Cin_g, Cout_g, k, stride, &a)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(dY) && radmmm::aligned16(W), "msd_gconv_dgrad: 16B alignment");
  a.slope = slope;
  const int jmax = (k - 1) / stride + 1;
  const int tc = Cin_g >= kChunk ? 1 : kChunk / Cin_g;
  const size_t lds = (size_t)((kRows - 1 + jmax) * (Cout_g + 4) + kSlack + Cout_g * (tc * Cin_g + 4) + kSlack) * sizeof(float);
  const int mrows = (Hin + k - 1 + stride - 1) / stride;       // rows of one phase
  hipLaunchKernelGGL(gconv_dgrad_kernel, dim3(((mrows + kRows - 1) / kRows) * stride, G, S), dim3(256), lds, ST(stream), dY, W, add,
                     X, dX, a);
  return radmmm::check_launch("msd_gconv_dgrad");
}

extern "C" int64_t radmmm_msd_gconv_wgrad_splits(int S, int Hout, int G, int k) {
  if (S <= 0 || Hout <= 0 || G <= 0 || k <= 0) return 0;
  const long long units = (long long)S * ((Hout + kRows - 1) / kRows);
  long long n = 1024 / ((long long)G * ((k + kWgradTaps - 1) / kWgradTaps));
  if (n > kMaxSplits) n = kMaxSplits;
  if (n > units) n = units;
  return n < 1 ? 1 : n;
}

extern "C" int radmmm_msd_gconv_wgrad(const float* dZ, const float* X, float* P, int S, int Hin, int Hout, int G, int Cin_g,
                                      int Cout_g, int k, int stride, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dZ && X && P, "msd_gconv_wgrad: null pointer");
  GconvArgs a;
  if (int rc = check_gconv("msd_gconv_wgrad", S, Hin, Hout, G, Cin_g, Cout_g, k, stride, &a)) return rc;
  const int nsplit = (int)radmmm_msd_gconv_wgrad_splits(S, Hout, G, k);
  RADMMM_REQUIRE((long long)nsplit * G * Cout_g * k * Cin_g * 4 < 0x7fffffffLL, "msd_gconv_wgrad: the partial sums exceed 2 GiB");
  RADMMM_REQUIRE(radmmm::aligned16(dZ) && radmmm::aligned16(X), "msd_gconv_wgrad: 16B alignment");
  const int rin = stride * (kRows - 1) + kWgradTaps;
  const size_t lds = (size_t)(kRows * (Cout_g + 4) + kSlack + rin * (Cin_g + 4) + kSlack) * sizeof(float);
  hipLaunchKernelGGL(gconv_wgrad_kernel, dim3((k + kWgradTaps - 1) / kWgradTaps, G, nsplit), dim3(256), lds, ST(stream), dZ, X, P, a,
                     nsplit);
  return radmmm::check_launch("msd_gconv_wgrad");
}

extern "C" int radmmm_msd_avgpool(const float* y, const float* y_hat, int ldy, float* out, int B, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(y && y_hat && out, "msd_avgpool: null pointer");
  RADMMM_REQUIRE(B > 0 && T > 0 && ldy >= T, "msd_avgpool: bad dims (B=%d T=%d ldy=%d)", B, T, ldy);
  const int To = T / 2 + 1;
  hipLaunchKernelGGL(avgpool_kernel, dim3(grid_for(2LL * B * To, 256)), dim3(256), 0, ST(stream), y, y_hat, ldy, out, B, T, To);
  return radmmm::check_launch("msd_avgpool");
}

extern "C" int radmmm_msd_avgpool_bwd(const float* g, float* gx, int ldx, int N, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(g && gx, "msd_avgpool_bwd: null pointer");
  RADMMM_REQUIRE(N > 0 && T > 0 && ldx >= T, "msd_avgpool_bwd: bad dims (N=%d T=%d ldx=%d)", N, T, ldx);
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(grid_for((long long)N * T, 256)), dim3(256), 0, ST(stream), g, gx, ldx, (long long)N, T,
                     T / 2 + 1);
  return radmmm::check_launch("msd_avgpool_bwd");
}

extern "C" int radmmm_msd_frame15(const float* y, const float* y_hat, int ldy, float* F, int B, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(y && y_hat && F, "msd_frame15: null pointer");
  RADMMM_REQUIRE(B > 0 && T > 0 && ldy >= T, "msd_frame15: bad dims (B=%d T=%d ldy=%d)", B, T, ldy);
  RADMMM_REQUIRE(2LL * B * T * 16 * 4 < 0x7fffffffLL, "msd_frame15: the frame matrix exceeds 2 GiB");
  hipLaunchKernelGGL(frame15_kernel, dim3(grid_for(2LL * B * T * 16, 256)), dim3(256), 0, ST(stream), y, y_hat, ldy, F, B, T);
  return radmmm::check_launch("msd_frame15");
}

extern "C" int radmmm_msd_unframe15(const float* dF, float* g, int ldg, int N, int T, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dF && g, "msd_unframe15: null pointer");
  RADMMM_REQUIRE(N > 0 && T > 0 && ldg >= T, "msd_unframe15: bad dims (N=%d T=%d ldg=%d)", N, T, ldg);
  RADMMM_REQUIRE((long long)N * T * 16 * 4 < 0x7fffffffLL, "msd_unframe15: the frame matrix exceeds 2 GiB");
  hipLaunchKernelGGL(unframe15_kernel, dim3(grid_for((long long)N * T, 256)), dim3(256), 0, ST(stream), dF, g, ldg, (long long)N, T);
  return radmmm::check_launch("msd_unframe15");
}

extern "C" int radmmm_msd_repad(const float* Z, int ldz, float* X, int S, int H, int C, int pad, float slope, radmmm_stream_t stream) {
  RADMMM_REQUIRE(Z && X, "msd_repad: null pointer");
  RADMMM_REQUIRE(S > 0 && H > 0 && C > 0 && C % 4 == 0 && pad >= 0 && pad <= 20,
                 "msd_repad: bad dims (S=%d H=%d C=%d pad=%d; C must be a multiple of 4, pad in [0, 20])", S, H, C, pad);
  RADMMM_REQUIRE((long long)S * (H + 2 * pad) * C * 4 < 0x7fffffffLL, "msd_repad: the map exceeds 2 GiB");
  RADMMM_REQUIRE(ldz % 4 == 0 && ldz >= C && radmmm::aligned16(Z) && radmmm::aligned16(X), "msd_repad: 16B alignment (ldz=%d)", ldz);
  hipLaunchKernelGGL(repad_kernel, dim3(grid_for((long long)S * (H + 2 * pad) * (C / 4), 256)), dim3(256), 0, ST(stream), Z, ldz, X,
                     (long long)S, H, C, pad, slope);
  return radmmm::check_launch("msd_repad");
}
