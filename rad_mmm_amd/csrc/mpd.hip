// HiFi-GAN multi-period discriminator (hifigan_models.py: DiscriminatorP / MultiPeriodDiscriminator) and the three GAN
// losses of loss.py on gfx950: what surrounds the row GEMMs of one discriminator.
//
// Layout.  One discriminator of period p sees S = 2 * B * p SEQUENCES: s = (sig * B + b) * p + w, sig 0 the real and 1 the
// generated signal, w the column of the fold x[b, h, w] = audio[b, h * p + w].  A feature map of C channels and H rows is a
// PADDED buffer [S][Hp][C], Hp = H + 4: two zero rows, the H rows, two zero rows.  A 5-tap window of stride st that starts
// at padded row st * h' is then one contiguous stretch of 5 * C floats (its taps are the rows st * h' - 2 .. st * h' + 2 of
// the map), which is the framed form of radmmm_rowgemm_f32 (a_item_stride = Hp * C, lda = st * C, K = 5 * C).  A DENSE
// matrix is [S * H][C].  The discriminator's output is [2B][H][p] (the reference's flatten: index h * p + w).
//
//   radmmm_mpd_fold_frame       audio -> frame matrix of the first conv (reflect tail, fold, windows): a copy
//   radmmm_mpd_repad            dense conv output -> leaky-relu -> padded map (pad rows written as zeros)
//   radmmm_mpd_frame            padded map -> explicit frame matrix [S * H'][5 * C] (the weight gradient's operand): a copy
//   radmmm_mpd_unframe          dFrames -> gradient of the conv input: adjoint of the framing in gather form (+ the map's own
//                               upstream gradient) times the leaky-relu derivative from the saved output
//   radmmm_mpd_conv_post        the 3-tap C -> 1 conv on a padded map
//   radmmm_mpd_conv_post_dgrad  its data gradient (+ upstream, times the derivative), dense
//   radmmm_mpd_conv_post_wgrad  partial rows of its weight and bias gradient (radmmm_colsum_final adds them)
//   radmmm_mpd_unfold_audio     gradient of the first conv's frames -> gradient of the audio (fold and reflect undone)
//   radmmm_mpd_fm_terms         masked partial sums of |r - g| of one map
//   radmmm_mpd_finish           partial sums + outputs -> the four loss terms and the normalisers, one workgroup, fp64
//   radmmm_mpd_fm_grad          gradient of the feature loss on one padded map
//   radmmm_mpd_out_grad         gradient of the adversarial terms (+ the feature loss) on the discriminator output
// The four loss kernels also serve the multi-scale discriminator (radmmm_msd_fm_terms / _finish / _fm_grad / _out_grad, DESIGN
// 4.23): the same kernels with p = 1, a pad parameter in place of the fixed 2 and eight maps in place of six.
// Every reduction has a fixed order and there are no atomics: equal inputs give equal bits.
#include "common.h"

namespace {

using radmmm::block_sum_f64;
using radmmm::grid_for;
using radmmm::lrelu;
using radmmm::ST;

constexpr int kTermsMaxBlocks = 1024;
constexpr int kFinishThreads = 1024;
constexpr int kPostRows = 64;   // rows per partial of conv_post_wgrad
constexpr int kMaxMaps = 8;     // maps of one discriminator, the output included

__device__ __forceinline__ int clamp_count(const int32_t* cnt, int b, int size) {
  if (!cnt) return size;
  const int n = cnt[b];
  return n < 0 ? 0 : (n > size ? size : n);
}

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// F[(s * H1 + h') * 8 + k] = x_s[3 h' - 2 + k] for k < 5 (0 outside [0, H)), 0 for k >= 5;  x_s[h] = audio[b][refl(h * p + w)]
__global__ void __launch_bounds__(256) fold_frame_kernel(const float* __restrict__ y, const float* __restrict__ yh, int ldy,
                                                         float* __restrict__ F, int B, int T, int p, int H, int H1) {
  const long long total = 2LL * B * p * H1 * 8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i & 7);
    const long long row = i >> 3;
    const int h1 = (int)(row % H1);
    const int s = (int)(row / H1);
    const int w = s % p, sb = s / p;
    const int sig = sb / B, b = sb - sig * B;
    const int h = 3 * h1 - 2 + k;
    float v = 0.f;
    if (k < 5 && h >= 0 && h < H) {
      int t = h * p + w;
      if (t >= T) t = 2 * (T - 1) - t;
      v = (sig ? yh : y)[(long long)b * ldy + t];
    }
    F[i] = v;
  }
}

// X[s][r][c] = 2 <= r < 2 + H ? lrelu(Z[(s * H + r - 2) * ldz + c]) : 0
__global__ void __launch_bounds__(256) repad_kernel(const float* __restrict__ Z, int ldz, float* __restrict__ X, long long S, int H,
                                                    int C, float slope) {
  const int q = C >> 2, Hp = H + 4;
  const long long total = S * Hp * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 4;
    const long long sr = i / q;
    const int r = (int)(sr % Hp);
    const long long s = sr / Hp;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= 2 && r < 2 + H) {
      v = *reinterpret_cast<const float4*>(Z + (s * H + r - 2) * ldz + c);
      v.x = lrelu(v.x, slope);
      v.y = lrelu(v.y, slope);
      v.z = lrelu(v.z, slope);
      v.w = lrelu(v.w, slope);
    }
    *reinterpret_cast<float4*>(X + sr * C + c) = v;
  }
}

// F[(s * Ho + h') * 5C + j] = X[(s * Hp + st * h') * C + j], j < 5C
__global__ void __launch_bounds__(256) frame_kernel(const float* __restrict__ X, float* __restrict__ F, long long S, int Hp, int C,
                                                    int Ho, int st) {
  const int q = 5 * C / 4;
  const long long total = S * Ho * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i % q) * 4;
    const long long row = i / q;
    const int h1 = (int)(row % Ho);
    const long long s = row / Ho;
    *reinterpret_cast<float4*>(F + row * 5 * C + j) = *reinterpret_cast<const float4*>(X + (s * Hp + (long long)st * h1) * C + j);
  }
}

// dZ[(s * H + h) * C + c] = (sum_{h'} dF[(s * Ho + h') * 5C + (h + 2 - st h') * C + c] + add[s][2 + h][c]) * lrelu'(X[s][2 + h][c])
// over the windows 0 <= h' < Ho with st h' <= h + 2 <= st h' + 4, ascending
__global__ void __launch_bounds__(256) unframe_kernel(const float* __restrict__ dF, const float* __restrict__ add,
                                                      const float* __restrict__ X, float* __restrict__ dZ, long long S, int H, int C,
                                                      int Ho, int st, float slope) {
  const int q = C >> 2, Hp = H + 4;
  const long long total = S * H * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 4;
    const long long row = i / q;
    const int h = (int)(row % H);
    const long long s = row / H;
    const int u = h + 2;
    int lo = u - 4 > 0 ? (u - 4 + st - 1) / st : 0;
    int hi = u / st;
    if (hi > Ho - 1) hi = Ho - 1;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int h1 = lo; h1 <= hi; ++h1) {
      const float4 t = *reinterpret_cast<const float4*>(dF + ((s * Ho + h1) * 5 + (u - st * h1)) * C + c);
      g.x += t.x; g.y += t.y; g.z += t.z; g.w += t.w;
    }
    const long long at = (s * Hp + u) * C + c;
    if (add) {
      const float4 t = *reinterpret_cast<const float4*>(add + at);
      g.x += t.x; g.y += t.y; g.z += t.z; g.w += t.w;
    }
    const float4 x = *reinterpret_cast<const float4*>(X + at);
    g.x *= x.x > 0.f ? 1.f : slope;
    g.y *= x.y > 0.f ? 1.f : slope;
    g.z *= x.z > 0.f ? 1.f : slope;
    g.w *= x.w > 0.f ? 1.f : slope;
    *reinterpret_cast<float4*>(dZ + row * C + c) = g;
  }
}

// out[(s2 * H + h) * p + w] = bias + sum_{k < 3} sum_c X[s2 * p + w][1 + h + k][c] * W[k * C + c]: one wave per output, lane l
// adds the float4 columns l, l + 64, ... tap by tap, then the xor butterfly
__global__ void __launch_bounds__(256) conv_post_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ out, long long n_out,
                                                        int p, int H, int C) {
  const int lane = threadIdx.x & 63;
  const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= n_out) return;
  const int w = (int)(o % p);
  const long long sh = o / p;
  const int h = (int)(sh % H);
  const long long s = (sh / H) * p + w;
  const float* x = X + (s * (H + 4) + 1 + h) * C;
  float acc = 0.f;
  for (int k = 0; k < 3; ++k)
    for (int c = lane * 4; c < C; c += 256) {
      const float4 a = *reinterpret_cast<const float4*>(x + (long long)k * C + c);
      const float4 b = *reinterpret_cast<const float4*>(W + k * C + c);
      acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
  acc = radmmm::wave_sum(acc);
  if (lane == 0) out[o] = acc + bias[0];
}

// dZ[(s * H + h) * C + c] = (sum_k dOut[s2][h + 1 - k][w] * W[k * C + c] + add[s][2 + h][c]) * lrelu'(X[s][2 + h][c])
__global__ void __launch_bounds__(256) conv_post_dgrad_kernel(const float* __restrict__ dOut, const float* __restrict__ W,
                                                              const float* __restrict__ add, const float* __restrict__ X,
                                                              float* __restrict__ dZ, long long S, int p, int H, int C, float slope) {
  const int q = C >> 2, Hp = H + 4;
  const long long total = S * H * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 4;
    const long long row = i / q;
    const int h = (int)(row % H);
    const long long s = row / H;
    const int w = (int)(s % p);
    const float* go = dOut + (s / p) * H * p + w;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < 3; ++k) {
      const int ho = h + 1 - k;
      if (ho < 0 || ho >= H) continue;
      const float d = go[(long long)ho * p];
      const float4 t = *reinterpret_cast<const float4*>(W + k * C + c);
      g.x += d * t.x; g.y += d * t.y; g.z += d * t.z; g.w += d * t.w;
    }
    const long long at = (s * Hp + 2 + h) * C + c;
    if (add) {
      const float4 t = *reinterpret_cast<const float4*>(add + at);
      g.x += t.x; g.y += t.y; g.z += t.z; g.w += t.w;
    }
    const float4 x = *reinterpret_cast<const float4*>(X + at);
    g.x *= x.x > 0.f ? 1.f : slope;
    g.y *= x.y > 0.f ? 1.f : slope;
    g.z *= x.z > 0.f ? 1.f : slope;
    g.w *= x.w > 0.f ? 1.f : slope;
    *reinterpret_cast<float4*>(dZ + row * C + c) = g;
  }
}

// part[j][k * C + c] = sum over the rows (s, h) of chunk j, ascending, of dOut[s2][h][w] * X[s][1 + h + k][c];
// part[j][3C] = the chunk's sum of dOut.  Row pitch 3C + 1.  Grid (chunks, ceil(3C / 256)): one column per thread.
__global__ void __launch_bounds__(256) conv_post_wgrad_kernel(const float* __restrict__ dOut, const float* __restrict__ X,
                                                              float* __restrict__ part, long long rows, int p, int H, int C) {
  __shared__ float d[kPostRows];
  __shared__ long long xrow[kPostRows];
  const long long r0 = (long long)blockIdx.x * kPostRows;
  const int n = (int)(r0 + kPostRows < rows ? kPostRows : rows - r0);
  if ((int)threadIdx.x < n) {
    const long long r = r0 + threadIdx.x;
    const long long s = r / H;
    const int h = (int)(r - s * H);
    d[threadIdx.x] = dOut[((s / p) * H + h) * p + (s % p)];
    xrow[threadIdx.x] = (s * (H + 4) + 1 + h) * C;
  }
  __syncthreads();
  float* out = part + (long long)blockIdx.x * (3 * C + 1);
  const int j = blockIdx.y * blockDim.x + threadIdx.x;
  if (j < 3 * C) {
    const int k = j / C, c = j - k * C;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += d[i] * X[xrow[i] + (long long)k * C + c];
    out[j] = acc;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += d[i];
    out[3 * C] = acc;
  }
}

// the windows of the first conv that hold folded position (h, w) of signal row sb, ascending
__device__ __forceinline__ float gather_fold(const float* __restrict__ dF, long long s, int h, int H1) {
  const int u = h + 2;
  int lo = u - 4 > 0 ? (u - 4 + 2) / 3 : 0;
  int hi = u / 3;
  if (hi > H1 - 1) hi = H1 - 1;
  float g = 0.f;
  for (int h1 = lo; h1 <= hi; ++h1) g += dF[(s * H1 + h1) * 8 + (u - 3 * h1)];
  return g;
}

// g[b][t] = own position t, then the mirrored tail position 2 (T - 1) - t when it lies in [T, H p)
__global__ void __launch_bounds__(256) unfold_audio_kernel(const float* __restrict__ dF, float* __restrict__ g, int ldg, int B,
                                                           int T, int p, int H, int H1, int sig) {
  const long long total = (long long)B * T;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / T), t = (int)(i - (long long)b * T);
    const long long s0 = ((long long)sig * B + b) * p;
    float v = gather_fold(dF, s0 + t % p, t / p, H1);
    const int m = 2 * (T - 1) - t;
    if (m >= T && m < H * p) v += gather_fold(dF, s0 + m % p, m / p, H1);
    g[(long long)b * ldg + t] = v;
  }
}

// element (b, w, h, c) of signal sig of a map: base + sig * ssig + b * sb + w * sw + h * sh + c
struct MapView {
  long long ssig, sb, sw, sh;
  int B, p, H, C;
};

// part[block] = sum of |r - g| over the block's elements with h < cnt[b]: thread-strided in a fixed order, then block_sum
__global__ void __launch_bounds__(256) fm_terms_kernel(const float* __restrict__ X, MapView v, const int32_t* __restrict__ cnt,
                                                       float* __restrict__ part) {
  __shared__ float sh[17];
  const int V = (v.C & 3) ? 1 : 4, q = v.C / V;
  const long long total = (long long)v.B * v.p * v.H * q;
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * V;
    long long r = i / q;
    const int h = (int)(r % v.H);
    r /= v.H;
    const int w = (int)(r % v.p), b = (int)(r / v.p);
    if (h >= clamp_count(cnt, b, v.H)) continue;
    const float* pr = X + b * v.sb + w * v.sw + h * v.sh + c;
    const float* pg = pr + v.ssig;
    if (V == 4) {
      const float4 a = *reinterpret_cast<const float4*>(pr);
      const float4 g = *reinterpret_cast<const float4*>(pg);
      acc += (fabsf(a.x - g.x) + fabsf(a.y - g.y)) + (fabsf(a.z - g.z) + fabsf(a.w - g.w));
    } else {
      acc += fabsf(pr[0] - pg[0]);
    }
  }
  acc = radmmm::block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// G (same layout as X) = +-coef * sign(r - g) * [h < cnt[b]], + on the real half; coef = up[0] / norm[0]
__global__ void __launch_bounds__(256) fm_grad_kernel(const float* __restrict__ X, MapView v, const int32_t* __restrict__ cnt,
                                                      const double* __restrict__ norm, const float* __restrict__ up,
                                                      float* __restrict__ G) {
  const int q = v.C >> 2;
  const long long total = (long long)v.B * v.p * v.H * q;
  const float coef = (float)((double)up[0] / norm[0]);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 4;
    long long r = i / q;
    const int h = (int)(r % v.H);
    r /= v.H;
    const int w = (int)(r % v.p), b = (int)(r / v.p);
    const long long at = b * v.sb + w * v.sw + h * v.sh + c;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (h < clamp_count(cnt, b, v.H)) {
      const float4 a = *reinterpret_cast<const float4*>(X + at);
      const float4 g = *reinterpret_cast<const float4*>(X + at + v.ssig);
      o = make_float4(coef * sign_of(a.x - g.x), coef * sign_of(a.y - g.y), coef * sign_of(a.z - g.z), coef * sign_of(a.w - g.w));
    }
    *reinterpret_cast<float4*>(G + at) = o;
    *reinterpret_cast<float4*>(G + at + v.ssig) = make_float4(-o.x, -o.y, -o.z, -o.w);
  }
}

struct FinishArgs {
  const float* part;   // the maps' partial sums, map l at [off[l], off[l + 1])
  int off[kMaxMaps + 1];
  int C[kMaxMaps];     // channels of the maps (the last is conv_post's: 1)
  int H[kMaxMaps];     // rows of the maps
  const float* out;    // [2B][H_post][p]
  const int32_t* cnt;  // [n + 1][B] or NULL: rows 0 .. n - 1 the maps' row counts, row n the output's count of flattened positions
  int B, p;
  int n;               // maps: 6 (multi-period), 8 (multi-scale)
};

// res = (fm, mean (1 - dr)^2, mean dg^2, mean (1 - dg)^2), norm[l] = sum_b cnt[l][b] * C_l * p (l < n), norm[n] = sum_b cnt[n][b]
__global__ void __launch_bounds__(kFinishThreads) finish_kernel(FinishArgs a, float* __restrict__ res, double* __restrict__ norm) {
  __shared__ double sh[kFinishThreads];
  const int H5 = a.H[a.n - 1], n = H5 * a.p;
  const int32_t* cnt_out = a.cnt ? a.cnt + a.n * a.B : nullptr;
  double fm = 0.0;
  for (int l = 0; l < a.n; ++l) {
    double s = 0.0, c = 0.0;
    for (int i = a.off[l] + threadIdx.x; i < a.off[l + 1]; i += kFinishThreads) s += (double)a.part[i];
    for (int b = threadIdx.x; b < a.B; b += kFinishThreads) c += (double)clamp_count(a.cnt ? a.cnt + l * a.B : nullptr, b, a.H[l]);
    s = block_sum_f64<kFinishThreads>(s, sh);
    c = block_sum_f64<kFinishThreads>(c, sh) * (double)a.C[l] * (double)a.p;
    if (threadIdx.x == 0) norm[l] = c;
    fm += s / c;
  }
  double r1 = 0.0, g0 = 0.0, g1 = 0.0, c = 0.0;
  const long long total = (long long)a.B * n;
  for (long long i = threadIdx.x; i < total; i += kFinishThreads) {
    const int b = (int)(i / n), f = (int)(i - (long long)b * n);
    if (f >= clamp_count(cnt_out, b, n)) continue;
    const double dr = (double)a.out[i], dg = (double)a.out[total + i];
    r1 += (1.0 - dr) * (1.0 - dr);
    g0 += dg * dg;
    g1 += (1.0 - dg) * (1.0 - dg);
  }
  for (int b = threadIdx.x; b < a.B; b += kFinishThreads) c += (double)clamp_count(cnt_out, b, n);
  r1 = block_sum_f64<kFinishThreads>(r1, sh);
  g0 = block_sum_f64<kFinishThreads>(g0, sh);
  g1 = block_sum_f64<kFinishThreads>(g1, sh);
  c = block_sum_f64<kFinishThreads>(c, sh);
  if (threadIdx.x == 0) {
    norm[a.n] = c;
    res[0] = (float)fm;
    res[1] = (float)(r1 / c);
    res[2] = (float)(g0 / c);
    res[3] = (float)(g1 / c);
  }
}

// dOut[sig][b][h][w]:  real = -2 (1 - dr) mf / n * up[1] + cf ;  generated = (2 dg up[2] - 2 (1 - dg) up[3]) mf / n - cf
// mf = [h p + w < cnt[nm][b]], n = norm[nm], cf = up[0] / norm[nm - 1] * sign(dr - dg) * [h < cnt[nm - 1][b]]; nm maps (6 or 8)
__global__ void __launch_bounds__(256) out_grad_kernel(const float* __restrict__ out, const int32_t* __restrict__ cnt,
                                                       const double* __restrict__ norm, const float* __restrict__ up,
                                                       float* __restrict__ dOut, int B, int p, int H, int nm) {
  const int n = H * p;
  const long long total = (long long)B * n;
  const float cfm = (float)((double)up[0] / norm[nm - 1]);
  const double inv = 1.0 / norm[nm];
  const float cr = (float)(-2.0 * (double)up[1] * inv), cg0 = (float)(2.0 * (double)up[2] * inv),
              cg1 = (float)(-2.0 * (double)up[3] * inv);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / n), f = (int)(i - (long long)b * n);
    const float dr = out[i], dg = out[total + i];
    const bool mf = f < clamp_count(cnt ? cnt + nm * B : nullptr, b, n);
    const bool mh = f / p < clamp_count(cnt ? cnt + (nm - 1) * B : nullptr, b, H);
    const float cf = mh ? cfm * sign_of(dr - dg) : 0.f;
    dOut[i] = (mf ? cr * (1.f - dr) : 0.f) + cf;
    dOut[total + i] = (mf ? cg0 * dg + cg1 * (1.f - dg) : 0.f) - cf;
  }
}

int check_map(const char* who, int S, int H, int C) {
  RADMMM_REQUIRE(S > 0 && H > 0 && C > 0 && C % 4 == 0, "%s: bad dims (S=%d H=%d C=%d; C must be a multiple of 4)", who, S, H, C);
  RADMMM_REQUIRE((long long)S * (H + 4) * C * 4 < 0x7fffffffLL, "%s: the map exceeds 2 GiB", who);
  return 0;
}

}  // namespace

extern "C" int radmmm_mpd_fold_frame(const float* y, const float* y_hat, int ldy, float* F, int B, int T, int p, int H, int H1,
                                     radmmm_stream_t stream) {
  RADMMM_REQUIRE(y && y_hat && F, "mpd_fold_frame: null pointer");
  RADMMM_REQUIRE(B > 0 && T > 0 && p > 0 && ldy >= T, "mpd_fold_frame: bad dims (B=%d T=%d p=%d ldy=%d)", B, T, p, ldy);
  RADMMM_REQUIRE(H == (T + p - 1) / p && H1 == (H - 1) / 3 + 1, "mpd_fold_frame: H=%d H1=%d do not belong to T=%d p=%d", H, H1, T, p);
  RADMMM_REQUIRE(H * p - T < T, "mpd_fold_frame: %d samples cannot be reflect-padded by %d", T, H * p - T);
  RADMMM_REQUIRE(2LL * B * p * H1 * 8 * 4 < 0x7fffffffLL, "mpd_fold_frame: the frame matrix exceeds 2 GiB");
  hipLaunchKernelGGL(fold_frame_kernel, dim3(grid_for(2LL * B * p * H1 * 8, 256)), dim3(256), 0, ST(stream), y, y_hat, ldy, F, B, T,
                     p, H, H1);
  return radmmm::check_launch("mpd_fold_frame");
}

extern "C" int radmmm_mpd_repad(const float* Z, int ldz, float* X, int S, int H, int C, float slope, radmmm_stream_t stream) {
  RADMMM_REQUIRE(Z && X, "mpd_repad: null pointer");
  if (int rc = check_map("mpd_repad", S, H, C)) return rc;
  RADMMM_REQUIRE(ldz % 4 == 0 && ldz >= C && radmmm::aligned16(Z) && radmmm::aligned16(X), "mpd_repad: 16B alignment (ldz=%d)", ldz);
  hipLaunchKernelGGL(repad_kernel, dim3(grid_for((long long)S * (H + 4) * (C / 4), 256)), dim3(256), 0, ST(stream), Z, ldz, X,
                     (long long)S, H, C, slope);
  return radmmm::check_launch("mpd_repad");
}

extern "C" int radmmm_mpd_frame(const float* X, float* F, int S, int H, int C, int Ho, int stride, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && F, "mpd_frame: null pointer");
  if (int rc = check_map("mpd_frame", S, H, C)) return rc;
  RADMMM_REQUIRE(stride >= 1 && Ho >= 1 && (long long)stride * (Ho - 1) + 5 <= H + 4, "mpd_frame: %d windows of stride %d leave the %d + 4 rows",
                 Ho, stride, H);
  RADMMM_REQUIRE((long long)S * Ho * 5 * C * 4 < 0x7fffffffLL, "mpd_frame: the frame matrix exceeds 2 GiB");
  RADMMM_REQUIRE(radmmm::aligned16(X) && radmmm::aligned16(F), "mpd_frame: 16B alignment");
  hipLaunchKernelGGL(frame_kernel, dim3(grid_for((long long)S * Ho * (5 * C / 4), 256)), dim3(256), 0, ST(stream), X, F, (long long)S,
                     H + 4, C, Ho, stride);
  return radmmm::check_launch("mpd_frame");
}

extern "C" int radmmm_mpd_unframe(const float* dF, const float* add, const float* X, float* dZ, int S, int H, int C, int Ho,
                                  int stride, float slope, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dF && X && dZ, "mpd_unframe: null pointer");
  if (int rc = check_map("mpd_unframe", S, H, C)) return rc;
  RADMMM_REQUIRE(stride >= 1 && Ho >= 1 && (long long)stride * (Ho - 1) + 5 <= H + 4, "mpd_unframe: %d windows of stride %d leave the %d + 4 rows",
                 Ho, stride, H);
  RADMMM_REQUIRE((long long)S * Ho * 5 * C * 4 < 0x7fffffffLL, "mpd_unframe: the frame matrix exceeds 2 GiB");
  RADMMM_REQUIRE(radmmm::aligned16(dF) && radmmm::aligned16(X) && radmmm::aligned16(dZ) && radmmm::aligned16(add),
                 "mpd_unframe: 16B alignment");
  hipLaunchKernelGGL(unframe_kernel, dim3(grid_for((long long)S * H * (C / 4), 256)), dim3(256), 0, ST(stream), dF, add, X, dZ,
                     (long long)S, H, C, Ho, stride, slope);
  return radmmm::check_launch("mpd_unframe");
}

extern "C" int radmmm_mpd_conv_post(const float* X, const float* W, const float* bias, float* out, int B2, int p, int H, int C,
                                    radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && W && bias && out, "mpd_conv_post: null pointer");
  RADMMM_REQUIRE(B2 > 0 && p > 0, "mpd_conv_post: bad dims (B2=%d p=%d)", B2, p);
  if (int rc = check_map("mpd_conv_post", B2 * p, H, C)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(X) && radmmm::aligned16(W), "mpd_conv_post: 16B alignment");
  const long long n_out = (long long)B2 * H * p;
  hipLaunchKernelGGL(conv_post_kernel, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, ST(stream), X, W, bias, out, n_out, p, H, C);
  return radmmm::check_launch("mpd_conv_post");
}

extern "C" int radmmm_mpd_conv_post_dgrad(const float* dOut, const float* W, const float* add, const float* X, float* dZ, int B2,
                                          int p, int H, int C, float slope, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dOut && W && X && dZ, "mpd_conv_post_dgrad: null pointer");
  RADMMM_REQUIRE(B2 > 0 && p > 0, "mpd_conv_post_dgrad: bad dims (B2=%d p=%d)", B2, p);
  if (int rc = check_map("mpd_conv_post_dgrad", B2 * p, H, C)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(W) && radmmm::aligned16(X) && radmmm::aligned16(dZ) && radmmm::aligned16(add),
                 "mpd_conv_post_dgrad: 16B alignment");
  const long long S = (long long)B2 * p;
  hipLaunchKernelGGL(conv_post_dgrad_kernel, dim3(grid_for(S * H * (C / 4), 256)), dim3(256), 0, ST(stream), dOut, W, add, X, dZ, S,
                     p, H, C, slope);
  return radmmm::check_launch("mpd_conv_post_dgrad");
}

extern "C" int64_t radmmm_mpd_conv_post_wgrad_parts(int B2, int p, int H) {
  return ((int64_t)B2 * p * H + kPostRows - 1) / kPostRows;
}

extern "C" int radmmm_mpd_conv_post_wgrad(const float* dOut, const float* X, float* part, int B2, int p, int H, int C,
                                          radmmm_stream_t stream) {
  RADMMM_REQUIRE(dOut && X && part, "mpd_conv_post_wgrad: null pointer");
  RADMMM_REQUIRE(B2 > 0 && p > 0, "mpd_conv_post_wgrad: bad dims (B2=%d p=%d)", B2, p);
  if (int rc = check_map("mpd_conv_post_wgrad", B2 * p, H, C)) return rc;
  const long long rows = (long long)B2 * p * H;
  hipLaunchKernelGGL(conv_post_wgrad_kernel, dim3((unsigned)radmmm_mpd_conv_post_wgrad_parts(B2, p, H), (3 * C + 255) / 256), dim3(256), 0, ST(stream),
                     dOut, X, part, rows, p, H, C);
  return radmmm::check_launch("mpd_conv_post_wgrad");
}

extern "C" int radmmm_mpd_unfold_audio(const float* dF, float* g, int ldg, int B, int T, int p, int H, int H1, int sig,
                                       radmmm_stream_t stream) {
  RADMMM_REQUIRE(dF && g, "mpd_unfold_audio: null pointer");
  RADMMM_REQUIRE(B > 0 && T > 0 && p > 0 && ldg >= T && (sig == 0 || sig == 1), "mpd_unfold_audio: bad dims (B=%d T=%d p=%d ldg=%d sig=%d)",
                 B, T, p, ldg, sig);
  RADMMM_REQUIRE(H == (T + p - 1) / p && H1 == (H - 1) / 3 + 1, "mpd_unfold_audio: H=%d H1=%d do not belong to T=%d p=%d", H, H1, T, p);
  RADMMM_REQUIRE(H * p - T < T, "mpd_unfold_audio: %d samples cannot be reflect-padded by %d", T, H * p - T);
  hipLaunchKernelGGL(unfold_audio_kernel, dim3(grid_for((long long)B * T, 256)), dim3(256), 0, ST(stream), dF, g, ldg, B, T, p, H, H1,
                     sig);
  return radmmm::check_launch("mpd_unfold_audio");
}

static int map_view(const char* who, int B, int p, int H, int C, int padded, int pad, MapView* v) {
  RADMMM_REQUIRE(B > 0 && p > 0 && H > 0 && C > 0, "%s: bad dims (B=%d p=%d H=%d C=%d)", who, B, p, H, C);
  RADMMM_REQUIRE(padded ? C % 4 == 0 : C == 1, "%s: a padded map needs C %% 4 == 0, the dense output C == 1 (C=%d)", who, C);
  RADMMM_REQUIRE(pad >= 0 && pad <= 20, "%s: pad must lie in [0, 20] (pad=%d)", who, pad);
  RADMMM_REQUIRE(2LL * B * p * (H + 2 * pad) * C * 4 < 0x7fffffffLL, "%s: the map exceeds 2 GiB", who);
  v->B = B; v->p = p; v->H = H; v->C = C;
  if (padded) {
    v->sh = C; v->sw = (long long)(H + 2 * pad) * C; v->sb = v->sw * p; v->ssig = v->sb * B;
  } else {
    v->sh = p; v->sw = 1; v->sb = (long long)H * p; v->ssig = v->sb * B;
  }
  return 0;
}

extern "C" int64_t radmmm_mpd_fm_terms_parts(int B, int p, int H, int C) {
  const int V = (C & 3) ? 1 : 4;
  return grid_for((long long)B * p * H * (C / V), 256, kTermsMaxBlocks);
}

static int fm_terms(const char* who, const float* X, const int32_t* cnt, float* part, int B, int p, int H, int C, int padded,
                    int pad, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && part, "%s: null pointer", who);
  MapView v;
  if (int rc = map_view(who, B, p, H, C, padded, pad, &v)) return rc;
  RADMMM_REQUIRE(!padded || radmmm::aligned16(X), "%s: 16B alignment", who);
  hipLaunchKernelGGL(fm_terms_kernel, dim3((unsigned)radmmm_mpd_fm_terms_parts(B, p, H, C)), dim3(256), 0, ST(stream),
                     padded ? X + pad * C : X, v, cnt, part);
  return radmmm::check_launch(who);
}

extern "C" int radmmm_mpd_fm_terms(const float* X, const int32_t* cnt, float* part, int B, int p, int H, int C, int padded,
                                   radmmm_stream_t stream) {
  return fm_terms("mpd_fm_terms", X, cnt, part, B, p, H, C, padded, 2, stream);
}

// pad >= 0: a map [2B][pad + H + pad][C]; pad < 0: the dense output [2B][H] (C == 1)
extern "C" int radmmm_msd_fm_terms(const float* X, const int32_t* cnt, float* part, int B, int H, int C, int pad,
                                   radmmm_stream_t stream) {
  return fm_terms("msd_fm_terms", X, cnt, part, B, 1, H, C, pad >= 0, pad >= 0 ? pad : 0, stream);
}

static int finish(const char* who, int n, const float* part, const int32_t* off, const int32_t* C, const int32_t* H, const float* out,
                  const int32_t* cnt, float* res, double* norm, int B, int p, radmmm_stream_t stream) {
  RADMMM_REQUIRE(part && off && C && H && out && res && norm, "%s: null pointer", who);
  RADMMM_REQUIRE(B > 0 && p > 0, "%s: bad dims (B=%d p=%d)", who, B, p);
  RADMMM_REQUIRE((reinterpret_cast<uintptr_t>(norm) & 7) == 0, "%s: norm must be 8B aligned", who);
  FinishArgs a = {};
  a.part = part; a.out = out; a.cnt = cnt; a.B = B; a.p = p; a.n = n;
  for (int l = 0; l <= n; ++l) a.off[l] = off[l];
  for (int l = 0; l < n; ++l) {
    RADMMM_REQUIRE(C[l] > 0 && H[l] > 0 && off[l + 1] >= off[l] && off[l] >= 0, "%s: bad map %d", who, l);
    a.C[l] = C[l];
    a.H[l] = H[l];
  }
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kFinishThreads), 0, ST(stream), a, res, norm);
  return radmmm::check_launch(who);
}

extern "C" int radmmm_mpd_finish(const float* part, const int32_t* off /* host [7] */, const int32_t* C /* host [6] */,
                                 const int32_t* H /* host [6] */, const float* out, const int32_t* cnt, float* res, double* norm,
                                 int B, int p, radmmm_stream_t stream) {
  return finish("mpd_finish", 6, part, off, C, H, out, cnt, res, norm, B, p, stream);
}

// eight maps (the seven convs and conv_post): off host [9], C and H host [8], cnt [9][B], norm [9]
extern "C" int radmmm_msd_finish(const float* part, const int32_t* off, const int32_t* C, const int32_t* H, const float* out,
                                 const int32_t* cnt, float* res, double* norm, int B, radmmm_stream_t stream) {
  return finish("msd_finish", 8, part, off, C, H, out, cnt, res, norm, B, 1, stream);
}

static int fm_grad(const char* who, const float* X, const int32_t* cnt, const double* norm, const float* up, float* G, int B, int p,
                   int H, int C, int pad, radmmm_stream_t stream) {
  RADMMM_REQUIRE(X && norm && up && G, "%s: null pointer", who);
  MapView v;
  if (int rc = map_view(who, B, p, H, C, 1, pad, &v)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(X) && radmmm::aligned16(G), "%s: 16B alignment", who);
  hipLaunchKernelGGL(fm_grad_kernel, dim3(grid_for((long long)B * p * H * (C / 4), 256)), dim3(256), 0, ST(stream), X + pad * C, v,
                     cnt, norm, up, G + pad * C);
  return radmmm::check_launch(who);
}

extern "C" int radmmm_mpd_fm_grad(const float* X, const int32_t* cnt, const double* norm, const float* up, float* G, int B, int p,
                                  int H, int C, radmmm_stream_t stream) {
  return fm_grad("mpd_fm_grad", X, cnt, norm, up, G, B, p, H, C, 2, stream);
}

extern "C" int radmmm_msd_fm_grad(const float* X, const int32_t* cnt, const double* norm, const float* up, float* G, int B, int H,
                                  int C, int pad, radmmm_stream_t stream) {
  return fm_grad("msd_fm_grad", X, cnt, norm, up, G, B, 1, H, C, pad, stream);
}

extern "C" int radmmm_mpd_out_grad(const float* out, const int32_t* cnt, const double* norm, const float* up, float* dOut, int B,
                                   int p, int H, radmmm_stream_t stream) {
  RADMMM_REQUIRE(out && norm && up && dOut, "mpd_out_grad: null pointer");
  RADMMM_REQUIRE(B > 0 && p > 0 && H > 0, "mpd_out_grad: bad dims (B=%d p=%d H=%d)", B, p, H);
  hipLaunchKernelGGL(out_grad_kernel, dim3(grid_for((long long)B * H * p, 256)), dim3(256), 0, ST(stream), out, cnt, norm, up, dOut,
                     B, p, H, 6);
  return radmmm::check_launch("mpd_out_grad");
}

// the eight-map form: cnt [9][B], norm [9]
extern "C" int radmmm_msd_out_grad(const float* out, const int32_t* cnt, const double* norm, const float* up, float* dOut, int B,
                                   int H, radmmm_stream_t stream) {
  RADMMM_REQUIRE(out && norm && up && dOut, "msd_out_grad: null pointer");
  RADMMM_REQUIRE(B > 0 && H > 0, "msd_out_grad: bad dims (B=%d H=%d)", B, H);
  hipLaunchKernelGGL(out_grad_kernel, dim3(grid_for((long long)B * H, 256)), dim3(256), 0, ST(stream), out, cnt, norm, up, dOut, B,
                     1, H, 8);
  return radmmm::check_launch("msd_out_grad");
}
