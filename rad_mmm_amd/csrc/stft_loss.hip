// Multi-resolution STFT loss (stft_loss.py: STFTLoss / MultiResolutionSTFTLoss) on gfx950: what surrounds the two row
// GEMMs of one resolution (frames x windowed DFT basis forward, dspec x basis^T backward).
//
// Layout.  A signal is [B][ldx] fp32 with T samples per item.  torch.stft(center=True) reflect-pads every item by
// h = n_fft / 2 at the padded length T and cuts F = 1 + T / hop frames of n_fft samples; the periodic hann window of `win`
// samples sits at columns [left, left + win), left = (n_fft - win) / 2, and is zero elsewhere.  Only those `win` columns
// are materialised: the frame matrix is [B*F][ldk] (ldk = roundup4(win)), row r = b*F + f, and the DFT's K is win.  The
// spectrum is [B*F][lds] with re in columns [0, cutoff) and im in [cutoff, 2 cutoff), cutoff = n_fft / 2 + 1.  `frames`
// is an int32 device array [B] of valid frames per item (clamped to [0, F] here); NULL means every frame is valid AND
// selects the reference's lens=None forms (global Frobenius ratio, plain mean).
//
//   radmmm_stftloss_frame    signal -> frame matrix (a copy: reflect about 0 and T-1), zeros in invalid rows / pad columns
//   radmmm_stftloss_terms    spectra -> per-frame partials (sum (ym-xm)^2, sum ym^2, sum |dlog|, 0), one wave per frame
//   radmmm_stftloss_finish   partials -> (sc, mag) of the resolution + the normalisers of the backward, one workgroup, fp64
//   radmmm_stftloss_bwd      spectra + partials + normalisers + upstream scalars -> dspec_x and / or dspec_y
//   radmmm_stftloss_unframe  dA [B*F][ldk] -> dx [B][lddx] (written or added to): the adjoint of frame in gather form
// Every reduction has a fixed order and there are no atomics: equal inputs give equal bits.
#include "common.h"

namespace {

using radmmm::block_sum_f64;
using radmmm::grid_for;
using radmmm::ST;

constexpr float kClamp = 1e-7f;   // torch.clamp(re^2 + im^2, min=1e-7)
constexpr int kRowsPerBlock = 4;  // one wave per frame row, four rows per workgroup
constexpr int kFinishThreads = 1024;

__device__ __forceinline__ int valid_frames(const int32_t* frames, int b, int F) {
  if (!frames) return F;
  const int n = frames[b];
  return n < 0 ? 0 : (n > F ? F : n);
}

// x[b][reflect(f*hop + left + j - h)] -> A[(b*F + f)*ldk + j]; four columns per thread
__global__ void __launch_bounds__(256) frame_kernel(const float* __restrict__ x, int ldx, const int32_t* __restrict__ frames,
                                                    float* __restrict__ A, int ldk, long long rows, int T, int F, int h,
                                                    int hop, int left, int win) {
  const int q = ldk >> 2;
  const long long total = rows * q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / q;
    const int j0 = (int)(i - r * q) * 4;
    const int b = (int)(r / F), f = (int)(r - (long long)b * F);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (f < valid_frames(frames, b, F)) {
      const float* xb = x + (long long)b * ldx;
      const int p0 = f * hop + left + j0 - h;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (j0 + e < win) {
          int p = p0 + e;
          p = p < 0 ? -p : p;
          p = p > T - 1 ? 2 * (T - 1) - p : p;
          v[e] = xb[p];
        }
      }
    }
    *reinterpret_cast<float4*>(A + r * ldk + j0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__device__ __forceinline__ float mag_of(float re, float im) { return sqrtf(fmaxf(re * re + im * im, kClamp)); }

// part[r] = (sum (ym - xm)^2, sum ym^2, sum |log ym - log xm|, 0): lane l adds bins l, l + 64, ... in order, then the
// wave's xor butterfly adds the 64 lane sums
__global__ void __launch_bounds__(64 * kRowsPerBlock) terms_kernel(const float* __restrict__ sx, const float* __restrict__ sy,
                                                                   int lds, const int32_t* __restrict__ frames,
                                                                   float* __restrict__ part, long long rows, int F, int cutoff,
                                                                   int a_weighting) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / F), f = (int)(r - (long long)b * F);
  float d = 0.f, n = 0.f, l = 0.f;
  if (f < valid_frames(frames, b, F)) {
    const float* px = sx + r * lds;
    const float* py = sy + r * lds;
    for (int k = lane; k < cutoff; k += 64) {
      const float xm = mag_of(px[k], px[cutoff + k]);
      const float ym = mag_of(py[k], py[cutoff + k]);
      const float e = ym - xm;
      d += e * e;
      n += ym * ym;
      l += a_weighting ? fabsf(logf(ym + 1.f) - logf(xm + 1.f)) : fabsf(logf(ym) - logf(xm));
    }
    d = radmmm::wave_sum(d);
    n = radmmm::wave_sum(n);
    l = radmmm::wave_sum(l);
  }
  if (lane == 0) *reinterpret_cast<float4*>(part + r * 4) = make_float4(d, n, l, 0.f);
}

// one workgroup: out = (sc, mag), norm = (S, sum D, sum N, 0) in fp64.  Ragged (frames != NULL): S = sum of the frame
// counts, sc = sum_r sqrt(D_r) / sqrt(N_r) / S, mag = sum_r L_r / (S * cutoff).  Global: S = rows,
// sc = sqrt(sum D) / sqrt(sum N), mag = sum L / (S * cutoff).
__global__ void __launch_bounds__(kFinishThreads) finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ frames,
                                                                float* __restrict__ out, double* __restrict__ norm, int B, int F,
                                                                int cutoff) {
  __shared__ double sh[kFinishThreads];
  const long long rows = (long long)B * F;
  double ratio = 0.0, dsum = 0.0, nsum = 0.0, lsum = 0.0, cnt = 0.0;
  for (long long r = threadIdx.x; r < rows; r += kFinishThreads) {
    const int b = (int)(r / F), f = (int)(r - (long long)b * F);
    if (f >= valid_frames(frames, b, F)) continue;
    const float4 p = *reinterpret_cast<const float4*>(part + r * 4);
    dsum += (double)p.x;
    nsum += (double)p.y;
    lsum += (double)p.z;
    ratio += sqrt((double)p.x) / sqrt((double)p.y);
  }
  for (int b = threadIdx.x; b < B; b += kFinishThreads) cnt += (double)valid_frames(frames, b, F);
  ratio = block_sum_f64<kFinishThreads>(ratio, sh);
  dsum = block_sum_f64<kFinishThreads>(dsum, sh);
  nsum = block_sum_f64<kFinishThreads>(nsum, sh);
  lsum = block_sum_f64<kFinishThreads>(lsum, sh);
  cnt = block_sum_f64<kFinishThreads>(cnt, sh);
  if (threadIdx.x == 0) {
    const double sc = frames ? ratio / cnt : sqrt(dsum) / sqrt(nsum);
    out[0] = (float)sc;
    out[1] = (float)(lsum / (cnt * (double)cutoff));
    norm[0] = cnt;
    norm[1] = dsum;
    norm[2] = nsum;
    norm[3] = 0.0;
  }
}

// d loss / d spec for one signal: (dre, dim) = dmag * (re, im) / mag where re^2 + im^2 >= 1e-7, else 0
__device__ __forceinline__ void store_bin(float* row, int cutoff, int k, float re, float im, float m, float dmag) {
  const bool pass = re * re + im * im >= kClamp;
  const float s = pass ? dmag / m : 0.f;
  row[k] = pass ? s * re : 0.f;
  row[cutoff + k] = pass ? s * im : 0.f;
}

__global__ void __launch_bounds__(64 * kRowsPerBlock) bwd_kernel(const float* __restrict__ sx, const float* __restrict__ sy, int lds,
                                                                 const float* __restrict__ part, const double* __restrict__ norm,
                                                                 const int32_t* __restrict__ frames, const float* __restrict__ g_sc,
                                                                 const float* __restrict__ g_mag, float scale, float* __restrict__ dsx,
                                                                 float* __restrict__ dsy, long long rows, int F, int cutoff,
                                                                 int a_weighting) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / F), f = (int)(r - (long long)b * F);
  float* ox = dsx ? dsx + r * lds : nullptr;
  float* oy = dsy ? dsy + r * lds : nullptr;
  if (f >= valid_frames(frames, b, F)) {
    for (int c = lane; c < lds; c += 64) {
      if (ox) ox[c] = 0.f;
      if (oy) oy[c] = 0.f;
    }
    return;
  }
  // wave-uniform coefficients in fp64
  const double S = norm[0];
  const double D = frames ? (double)part[r * 4 + 0] : norm[1];
  const double N = frames ? (double)part[r * 4 + 1] : norm[2];
  const double csc = (double)g_sc[0] * (double)scale / (frames ? S : 1.0);
  const double sd = sqrt(D), sn = sqrt(N);
  const float c_diff = (float)(D > 0.0 ? csc / (sd * sn) : 0.0);   // the norm's gradient at 0 is 0
  const float c_y = (float)(csc * sd / (N * sn));
  const float c_log = (float)((double)g_mag[0] * (double)scale / (S * (double)cutoff));
  const float* px = sx + r * lds;
  const float* py = sy + r * lds;
  for (int k = lane; k < cutoff; k += 64) {
    const float xr = px[k], xi = px[cutoff + k], yr = py[k], yi = py[cutoff + k];
    const float xm = mag_of(xr, xi), ym = mag_of(yr, yi);
    const float dl = a_weighting ? logf(ym + 1.f) - logf(xm + 1.f) : logf(ym) - logf(xm);
    const float sg = dl > 0.f ? c_log : (dl < 0.f ? -c_log : 0.f);
    const float e = ym - xm;
    if (ox) store_bin(ox, cutoff, k, xr, xi, xm, -c_diff * e - sg / (a_weighting ? xm + 1.f : xm));
    if (oy) store_bin(oy, cutoff, k, yr, yi, ym, c_diff * e - c_y * ym + sg / (a_weighting ? ym + 1.f : ym));
  }
  for (int c = 2 * cutoff + lane; c < lds; c += 64) {
    if (ox) ox[c] = 0.f;
    if (oy) oy[c] = 0.f;
  }
}

// sum of dA over the frames f < nf that hold padded position P (column P - left - f*hop in [0, win)), f ascending
__device__ __forceinline__ float gather_position(const float* __restrict__ dAb, int ldk, int P, int nf, int hop, int left,
                                                 int win) {
  const int u = P - left;   // f*hop <= u <= f*hop + win - 1
  if (u < 0) return 0.f;
  int f_hi = u / hop;
  if (f_hi > nf - 1) f_hi = nf - 1;
  const int lo = u - win + 1;
  const int f_lo = lo > 0 ? (lo + hop - 1) / hop : 0;
  float s = 0.f;
  for (int f = f_lo; f <= f_hi; ++f) s += dAb[(long long)f * ldk + (u - f * hop)];
  return s;
}

// dx[b][s] = own position s + h, then the left mirror h - s (1 <= s <= h), then the right mirror h + 2(T-1) - s
// (T-1-h <= s <= T-2)
__global__ void __launch_bounds__(256) unframe_kernel(const float* __restrict__ dA, int ldk, const int32_t* __restrict__ frames,
                                                      float* __restrict__ dx, int lddx, int B, int T, int F, int h, int hop,
                                                      int left, int win, int accum) {
  const long long total = (long long)B * T;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / T), s = (int)(i - (long long)b * T);
    const int nf = valid_frames(frames, b, F);
    const float* dAb = dA + (long long)b * F * ldk;
    float g = gather_position(dAb, ldk, s + h, nf, hop, left, win);
    if (s >= 1 && s <= h) g += gather_position(dAb, ldk, h - s, nf, hop, left, win);
    if (s >= T - 1 - h && s <= T - 2) g += gather_position(dAb, ldk, h + 2 * (T - 1) - s, nf, hop, left, win);
    float* o = dx + (long long)b * lddx + s;
    *o = accum ? *o + g : g;
  }
}

// the shape of one resolution: n_fft even, 1 <= win <= n_fft, hop >= 1, T > n_fft / 2 (the reflect pad), F frames
int check_shape(const char* who, int B, int T, int F, int n_fft, int hop, int win, int ldk) {
  RADMMM_REQUIRE(B > 0 && T > 0 && n_fft >= 2 && n_fft % 2 == 0 && hop >= 1 && win >= 1, "%s: bad dims (B=%d T=%d n_fft=%d hop=%d win=%d)",
                 who, B, T, n_fft, hop, win);
  RADMMM_REQUIRE(win <= n_fft, "%s: win=%d exceeds n_fft=%d", who, win, n_fft);
  RADMMM_REQUIRE(T > n_fft / 2, "%s: T=%d cannot be reflect-padded by n_fft/2=%d", who, T, n_fft / 2);
  RADMMM_REQUIRE(F >= 1 && F <= 1 + T / hop, "%s: F=%d frames, at most 1 + T / hop = %d", who, F, 1 + T / hop);
  RADMMM_REQUIRE(ldk % 4 == 0 && ldk >= win, "%s: ldk=%d must be a multiple of 4 and >= win=%d", who, ldk, win);
  RADMMM_REQUIRE((long long)B * F * ldk * 4 < 0x7fffffffLL, "%s: the frame matrix exceeds 2 GiB", who);
  return 0;
}

int check_spec(const char* who, int B, int F, int cutoff, int lds) {
  RADMMM_REQUIRE(B > 0 && F > 0 && cutoff > 0, "%s: bad dims (B=%d F=%d cutoff=%d)", who, B, F, cutoff);
  RADMMM_REQUIRE(lds % 4 == 0 && lds >= 2 * cutoff, "%s: lds=%d must be a multiple of 4 and >= 2 * cutoff=%d", who, lds, 2 * cutoff);
  RADMMM_REQUIRE((long long)B * F * lds * 4 < 0x7fffffffLL, "%s: the spectrum exceeds 2 GiB", who);
  return 0;
}

}  // namespace

extern "C" int radmmm_stftloss_frame(const float* x, int ldx, const int32_t* frames, float* A, int ldk, int B, int T, int F,
                                     int n_fft, int hop, int win, radmmm_stream_t stream) {
  RADMMM_REQUIRE(x && A, "stftloss_frame: null pointer");
  if (int rc = check_shape("stftloss_frame", B, T, F, n_fft, hop, win, ldk)) return rc;
  RADMMM_REQUIRE(ldx >= T, "stftloss_frame: ldx=%d < T=%d", ldx, T);
  RADMMM_REQUIRE(radmmm::aligned16(A), "stftloss_frame: A must be 16B aligned");
  const long long rows = (long long)B * F;
  hipLaunchKernelGGL(frame_kernel, dim3(grid_for(rows * (ldk / 4), 256)), dim3(256), 0, ST(stream), x, ldx, frames, A, ldk,
                     rows, T, F, n_fft / 2, hop, (n_fft - win) / 2, win);
  return radmmm::check_launch("stftloss_frame");
}

extern "C" int radmmm_stftloss_terms(const float* spec_x, const float* spec_y, int lds, const int32_t* frames, float* part,
                                     int B, int F, int cutoff, int a_weighting, radmmm_stream_t stream) {
  RADMMM_REQUIRE(spec_x && spec_y && part, "stftloss_terms: null pointer");
  if (int rc = check_spec("stftloss_terms", B, F, cutoff, lds)) return rc;
  RADMMM_REQUIRE(radmmm::aligned16(part), "stftloss_terms: part must be 16B aligned");
  const long long rows = (long long)B * F;
  hipLaunchKernelGGL(terms_kernel, dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(64 * kRowsPerBlock), 0,
                     ST(stream), spec_x, spec_y, lds, frames, part, rows, F, cutoff, a_weighting);
  return radmmm::check_launch("stftloss_terms");
}

extern "C" int radmmm_stftloss_finish(const float* part, const int32_t* frames, float* out, double* norm, int B, int F,
                                      int cutoff, radmmm_stream_t stream) {
  RADMMM_REQUIRE(part && out && norm, "stftloss_finish: null pointer");
  RADMMM_REQUIRE(B > 0 && F > 0 && cutoff > 0, "stftloss_finish: bad dims (B=%d F=%d cutoff=%d)", B, F, cutoff);
  RADMMM_REQUIRE(radmmm::aligned16(part), "stftloss_finish: part must be 16B aligned");
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kFinishThreads), 0, ST(stream), part, frames, out, norm, B, F, cutoff);
  return radmmm::check_launch("stftloss_finish");
}

extern "C" int radmmm_stftloss_bwd(const float* spec_x, const float* spec_y, int lds, const float* part, const double* norm,
                                   const int32_t* frames, const float* g_sc, const float* g_mag, float scale, float* dspec_x,
                                   float* dspec_y, int B, int F, int cutoff, int a_weighting, radmmm_stream_t stream) {
  RADMMM_REQUIRE(spec_x && spec_y && part && norm && g_sc && g_mag && (dspec_x || dspec_y), "stftloss_bwd: null pointer");
  if (int rc = check_spec("stftloss_bwd", B, F, cutoff, lds)) return rc;
  const long long rows = (long long)B * F;
  hipLaunchKernelGGL(bwd_kernel, dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(64 * kRowsPerBlock), 0,
                     ST(stream), spec_x, spec_y, lds, part, norm, frames, g_sc, g_mag, scale, dspec_x, dspec_y, rows, F, cutoff,
                     a_weighting);
  return radmmm::check_launch("stftloss_bwd");
}

extern "C" int radmmm_stftloss_unframe(const float* dA, int ldk, const int32_t* frames, float* dx, int lddx, int B, int T,
                                       int F, int n_fft, int hop, int win, int accum, radmmm_stream_t stream) {
  RADMMM_REQUIRE(dA && dx, "stftloss_unframe: null pointer");
  if (int rc = check_shape("stftloss_unframe", B, T, F, n_fft, hop, win, ldk)) return rc;
  RADMMM_REQUIRE(lddx >= T, "stftloss_unframe: lddx=%d < T=%d", lddx, T);
  hipLaunchKernelGGL(unframe_kernel, dim3(grid_for((long long)B * T, 256)), dim3(256), 0, ST(stream), dA, ldk, frames, dx, lddx,
                     B, T, F, n_fft / 2, hop, (n_fft - win) / 2, win, accum);
  return radmmm::check_launch("stftloss_unframe");
}
