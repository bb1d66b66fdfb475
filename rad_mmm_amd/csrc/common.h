// Shared helpers for libradmmm_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/radmmm_hip.h"

namespace radmmm {

void set_error(const char* fmt, ...);
// value of an experiment / test switch, or nullptr unless RADMMM_DEBUG=1 (error.cpp)
const char* debug_env(const char* name);

// The fp32 GEMM family (radmmm_rowgemm_f32 / radmmm_wgrad_f32): ONE host decision, gemm_f32.hip plan_rowgemm_f32 /
// plan_wgrad_f32 (validation, kernel family, tiling, buffer extents; no HIP call).  The entry points launch what it says and
// radmmm_rowgemm_f32_plan / radmmm_wgrad_f32_plan report it.
struct f32_plan {
  int family;            // RADMMM_F32_FAMILY_*
  int bl;                // b_layout (row GEMMs)
  int mt, rows, nmt;     // 16-row kernel: tile height / 16, rows per tile, number of row tiles; 0 otherwise
  int ntn;               // column tiles of 128 (row GEMMs)
  int a_bytes, b_bytes;  // byte extents of the buffer descriptors (A / B of rowgemm16, GY / X of wgrad16)
};
constexpr int kMixNK = 160;       // the channel mix kernel's N = K (rowgemm_mix.hip)
constexpr int kWgrad16BK = 16;    // frames per K step of wgrad16 (wgrad16_f32.hip)
int plan_rowgemm_f32(const radmmm_rowgemm_desc* d, f32_plan* pl);   // 0, or < 0 with the error string set
int plan_wgrad_f32(const radmmm_wgrad_desc* d, f32_plan* pl);
int launch_rowgemm16(const radmmm_rowgemm_desc& d, const f32_plan& pl, hipStream_t stream);    // rowgemm16_f32.hip
int launch_rowgemm_mix(const radmmm_rowgemm_desc& d, const f32_plan& pl, hipStream_t stream);  // rowgemm_mix.hip
int launch_wgrad16(const radmmm_wgrad_desc& d, const f32_plan& pl, hipStream_t stream);        // wgrad16_f32.hip

// The split-operand row GEMM (radmmm_rowgemm_h3): ONE host decision, rowgemm_h3w.hip plan_rowgemm_h3 (validation, buffer
// extents, narrow or wide tile, tile height, epilogue kind, kernel family, every RADMMM_DEBUG switch of the family; its only
// HIP call is gemm_cu_slots()'s once-per-process query).  The entry point launches what it says, radmmm_rowgemm_h3_plan and
// radmmm_rowgemm_h3_colsum_rows report it.
struct h3_plan {
  int family;            // RADMMM_H3_FAMILY_*
  int products;          // 1 / 2 / 3 (nprod 0 reads as 3)
  int mb, ek;            // tile height / 32 and epilogue kind EK_* (rowgemm_h3_tiles.h); the narrow kernel: 4 and 0
  int a_bytes, b_bytes;  // byte extents of the operands' buffer descriptors
  int colsum_rows;       // partial rows a direct epilogue leaves in colsum_scratch; 0: the narrow kernel, the generic epilogue
};
int plan_rowgemm_h3(const radmmm_rowgemm_h3_desc* d, h3_plan* pl);   // 0, or < 0 with the error string set
int launch_rowgemm_h3_narrow(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream);   // rowgemm_h3.hip
int launch_h3d_pr1(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream);   // rowgemm_h3w_pr{1,2,3}.hip: all (tile
int launch_h3d_pr2(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream);   // height, epilogue kind) instantiations
int launch_h3d_pr3(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream);   // of one product scheme
int launch_rowgemm_win(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream);   // rowgemm_win.hip
int launch_rowgemm_one(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream);   // rowgemm_one.hip
int gemm_cu_slots();
// the kernel the calling thread's last radmmm_rowgemm_h3 launch took (radmmm_rowgemm_h3_last_kernel; error.cpp)
extern thread_local int g_h3_last_kernel;

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return -2;
  }
  return 0;
}

#define RADMMM_REQUIRE(cond, ...)      \
  do {                                 \
    if (!(cond)) {                     \
      radmmm::set_error(__VA_ARGS__);  \
      return -1;                       \
    }                                  \
  } while (0)

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline hipStream_t ST(radmmm_stream_t s) { return static_cast<hipStream_t>(s); }

// workgroups of a grid-stride launch over `total` elements.  The cap is part of a kernel's result wherever the grid fixes the
// order of a reduction: files with another cap (elementwise.hip, film.hip, synth.hip, stft_kernels.h, waveglow.hip) keep their own.
inline int grid_for(long long total, int block, int cap = 8192) {
  long long g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// The frame-shift origin of the row-major weight-gradient kernels (wgrad_rm.hip, wgrad_rm8.hip): the largest shift0 they take.
// Their mask rule holds for ANY shift -- a row's partner frame f + shift is tested against the readable range [0, lim) of the
// row's OWN utterance, and a row that fails has its DMA offset replaced by an out-of-range one whatever it was -- so a
// readable row's offset always lies inside the operand.  What is left is the arithmetic: a lane forms (f + shift) * ldx * 2
// in 32 bits for every row, readable or not, with f up to R + 96 (the last window's rows and the two steps the DMA runs
// ahead).  The bound keeps that product of an unreadable row from leaving the signed range.  The tap shifts of the plain
// entry points (up to 2 * 128 frames in the WaveGlow WN) are as they were: the check is made for shift0 != 0 only.
inline bool wgrad_rm_shift_fits(int R, int ldx, int shift0, int taps, int dil) {
  const long long reach = (shift0 < 0 ? -(long long)shift0 : (long long)shift0) + (long long)(taps / 2) * dil;
  return shift0 == 0 || ((long long)R + 96 + reach) * ldx * 2 <= 0x7fffffffLL;
}

// ---- device helpers -------------------------------------------------------------
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for vmcnt(0), i.e. for the
// write acknowledgements of every global store issued so far (stores count in vmcnt on gfx9): in an
// epilogue that alternates "stage a block in LDS / store it" that costs one HBM write round trip (2-5 us)
// per block.  Use only where no global-memory hand-off between the waves depends on the barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float softplus_f(float x) {
  // torch.nn.Softplus(beta=1, threshold=20): x > 20 ? x : log1p(exp(x)) = max(x, 0) + log1p(exp(-|x|)).
  // Hardware exp2/log2 (v_exp_f32 / v_log_f32, 1 ulp) instead of libm's expf/log1pf: ~12 VALU
  // instructions instead of ~100, which matters because the GEMM epilogues are VALU bound.
  // log1p(e) = log(u) * e / (u - 1) with u = fl(1 + e) keeps full relative accuracy for small e.
  const float e = __expf(-fabsf(x));
  const float u = 1.f + e;
  const float d = u - 1.f;
  const float l = (d == 0.f) ? e : __logf(u) * __fdividef(e, d);
  return x > 20.f ? x : fmaxf(x, 0.f) + l;
}
// 1 - exp(-y) for y >= 0 without cancellation for small y
__device__ __forceinline__ float one_minus_exp_neg(float y) {
  const float p = y * (1.f - y * (0.5f - y * (0.16666667f - y * (0.041666668f - y * (0.0083333338f - y * 0.0013888889f)))));
  return y < 0.25f ? p : 1.f - __expf(-y);
}
__device__ __forceinline__ float act_apply(float v, int act) {
  switch (act) {
    case RADMMM_ACT_SOFTPLUS: return softplus_f(v);
    case RADMMM_ACT_RELU: return v > 0.f ? v : 0.f;
    case RADMMM_ACT_LEAKY: return v > 0.f ? v : 0.01f * v;
    default: return v;
  }
}
// derivative of the activation expressed from its OUTPUT y
__device__ __forceinline__ float dact_from_out(float y, int act) {
  switch (act) {
    case RADMMM_ACT_SOFTPLUS: return y > 20.f ? 1.f : one_minus_exp_neg(y);  // sigmoid(x) = 1 - exp(-softplus(x))
    case RADMMM_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case RADMMM_ACT_LEAKY: return y > 0.f ? 1.f : 0.01f;
    default: return 1.f;
  }
}
// partial-conv renormalisation ratio for frame t of an item with `len` valid frames
// (partialconv1d.py:75-81): taps/(cnt+1e-6) * clamp(cnt,0,1)
__device__ __forceinline__ float pconv_ratio(int t, int len, int taps, int dil) {
  int cnt = 0;
  const int c = taps / 2;
  for (int k = 0; k < taps; ++k) {
    const int ts = t + (k - c) * dil;
    cnt += (ts >= 0 && ts < len) ? 1 : 0;
  }
  return cnt > 0 ? (float)taps / ((float)cnt + 1e-6f) : 0.f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// block-wide sum for blockDim.x <= 1024 (multiple of 64); result valid in all threads
__device__ __forceinline__ float block_sum(float v, float* sh /* >= 17 floats */) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  if (w == 0) {
    float t = lane < nw ? sh[lane] : 0.f;
    t = wave_sum(t);
    if (lane == 0) sh[16] = t;
  }
  __syncthreads();
  return sh[16];
}

// block-wide fp64 sum in a fixed tree order for a workgroup of exactly N threads (a power of two); result valid in all threads
template <int N>
__device__ __forceinline__ double block_sum_f64(double v, double* sh /* N doubles */) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = N / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }

// weight of row r in a (bias-gradient) column sum: 0 none, 1 length mask, 2 mask x partial-conv ratio
__device__ __forceinline__ float colsum_row_weight(int r, int row_weight, int T, const int* lens, int taps,
                                                   int dil) {
  if (!row_weight) return 1.f;
  const int b = r / T, t = r - b * T;
  const int len = lens ? lens[b] : T;
  if (t >= len) return 0.f;
  if (row_weight != 2) return 1.f;
  int cnt = 0;
  for (int k = 0; k < taps; ++k) {
    const int ts = t + (k - taps / 2) * dil;
    cnt += (ts >= 0 && ts < len) ? 1 : 0;
  }
  return ((float)cnt + 1e-6f) / (float)taps;
}

}  // namespace radmmm
