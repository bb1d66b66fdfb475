// Optimizer step on flat fp32 buffers: the reference's vendored RAdam
// (radam.py:63-142) fused with Lightning's global-norm gradient clip
// (configs/RADMMM_train_config.yaml:7-8).  Parameters, gradients and both moments of one
// bucket are contiguous arrays (rad_mmm_amd/optim.py makes the parameters views of a flat buffer,
// as ddp.py already does for the gradients), so the whole update of 26.5 M parameters is one
// streaming kernel: 4 reads + 3 writes per element, HBM bound.
#include "common.h"

namespace {

constexpr int SUMSQ_BLOCKS = 1024;

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, long long n, float* __restrict__ part) {
  __shared__ float sh[17];
  float s = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(x + i);
      s = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, s))));
    } else {
      for (long long k = i; k < n; ++k) s = fmaf(x[k], x[k], s);
    }
  }
  s = radmmm::block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// clip[0] (device scalar, may be null) multiplies the gradient; use_denom: N_sma >= 5 branch
struct RAdamCoef {
  float c, beta1, beta2, eps, step_size, wd_lr;
  int use_denom;
};
__device__ __forceinline__ void radam_one(float& pi, float gi, float& mi, float& vi, const RAdamCoef& k) {
  gi *= k.c;
  vi = vi * k.beta2 + (1.f - k.beta2) * gi * gi;
  mi = mi * k.beta1 + (1.f - k.beta1) * gi;
  pi += -k.wd_lr * pi;
  pi += k.use_denom ? -k.step_size * (mi / (sqrtf(vi) + k.eps)) : -k.step_size * mi;
}
// 28 bytes of HBM traffic per parameter and nothing else: four parameters per lane and access (16-byte loads / stores,
// streaming: every byte is touched once per step and the four arrays together are far larger than the last-level cache)
__global__ __launch_bounds__(256) void radam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long long n,
                                                    const float* __restrict__ clip, float beta1, float beta2, float eps,
                                                    float step_size, float wd_lr, int use_denom) {
  const RAdamCoef k{clip ? clip[0] : 1.f, beta1, beta2, eps, step_size, wd_lr, use_denom};
  const long long stride = (long long)gridDim.x * blockDim.x, tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = n >> 2;
  using f4 = __attribute__((ext_vector_type(4))) float;
  f4* p4 = reinterpret_cast<f4*>(p);
  f4* m4 = reinterpret_cast<f4*>(m);
  f4* v4 = reinterpret_cast<f4*>(v);
  const f4* g4 = reinterpret_cast<const f4*>(g);
  for (long long i = tid; i < n4; i += stride) {
    const f4 gi = __builtin_nontemporal_load(g4 + i);
    const f4 pv = __builtin_nontemporal_load(p4 + i), mv = __builtin_nontemporal_load(m4 + i), vv = __builtin_nontemporal_load(v4 + i);
    float pj[4], mj[4], vj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pj[j] = pv[j];
      mj[j] = mv[j];
      vj[j] = vv[j];
      radam_one(pj[j], gi[j], mj[j], vj[j], k);
    }
    __builtin_nontemporal_store(f4{vj[0], vj[1], vj[2], vj[3]}, v4 + i);
    __builtin_nontemporal_store(f4{mj[0], mj[1], mj[2], mj[3]}, m4 + i);
    __builtin_nontemporal_store(f4{pj[0], pj[1], pj[2], pj[3]}, p4 + i);
  }
  for (long long i = (n4 << 2) + tid; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    radam_one(pi, g[i], mi, vi, k);
    v[i] = vi;
    m[i] = mi;
    p[i] = pi;
  }
}

// torch.optim.Adam / AdamW (single-tensor form) on a flat fp32 bucket.  The scalars of a step come from the device step
// counter, in double, once per thread; a raised skip word ends every thread before it touches p, g, m or v.
struct AdamCoef {
  float c, b1, omb1, b2, omb2, eps, step_size, bc2_sqrt, decay, wd;
  int decoupled;
};
__device__ __forceinline__ double ipow(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}
__device__ __forceinline__ void adam_one(float& pi, float gi, float& mi, float& vi, const AdamCoef& k) {
  gi *= k.c;
  if (k.decoupled)
    pi *= k.decay;
  else if (k.wd != 0.f)
    gi += k.wd * pi;
  mi = k.b1 * mi + k.omb1 * gi;
  vi = k.b2 * vi + k.omb2 * gi * gi;
  pi -= k.step_size * (mi / (sqrtf(vi) / k.bc2_sqrt + k.eps));
}
__global__ void adam_advance_kernel(int* __restrict__ step, const int* __restrict__ skip) {
  if (skip && skip[0] != 0) return;
  step[0] += 1;
}
// the traffic and the access pattern of radam_kernel: 28 bytes per parameter, 16-byte streaming loads / stores
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n, const float* __restrict__ clip,
                                                   const int* __restrict__ step, const int* __restrict__ skip, double lr,
                                                   double beta1, double beta2, double eps, double wd, int decoupled) {
  if (skip && skip[0] != 0) return;
  const int t = step[0];                                   // the count AFTER this step (adam_advance_kernel ran before)
  const double bc1 = 1.0 - ipow(beta1, t), bc2 = 1.0 - ipow(beta2, t);
  const AdamCoef k{clip ? clip[0] : 1.f, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                   (float)(lr / bc1), (float)sqrt(bc2), (float)(1.0 - lr * wd), (float)wd, decoupled};
  const long long stride = (long long)gridDim.x * blockDim.x, tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = n >> 2;
  using f4 = __attribute__((ext_vector_type(4))) float;
  f4* p4 = reinterpret_cast<f4*>(p);
  f4* m4 = reinterpret_cast<f4*>(m);
  f4* v4 = reinterpret_cast<f4*>(v);
  const f4* g4 = reinterpret_cast<const f4*>(g);
  for (long long i = tid; i < n4; i += stride) {
    const f4 gi = __builtin_nontemporal_load(g4 + i);
    const f4 pv = __builtin_nontemporal_load(p4 + i), mv = __builtin_nontemporal_load(m4 + i), vv = __builtin_nontemporal_load(v4 + i);
    float pj[4], mj[4], vj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pj[j] = pv[j];
      mj[j] = mv[j];
      vj[j] = vv[j];
      adam_one(pj[j], gi[j], mj[j], vj[j], k);
    }
    __builtin_nontemporal_store(f4{vj[0], vj[1], vj[2], vj[3]}, v4 + i);
    __builtin_nontemporal_store(f4{mj[0], mj[1], mj[2], mj[3]}, m4 + i);
    __builtin_nontemporal_store(f4{pj[0], pj[1], pj[2], pj[3]}, p4 + i);
  }
  for (long long i = (n4 << 2) + tid; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_one(pi, g[i], mi, vi, k);
    v[i] = vi;
    m[i] = mi;
    p[i] = pi;
  }
}

}  // namespace

extern "C" int64_t radmmm_sumsq_scratch_floats(void) { return SUMSQ_BLOCKS; }

// partial[0 .. radmmm_sumsq_scratch_floats()) = per-block sums of x^2 (the caller adds them; no atomics)
extern "C" int radmmm_sumsq(const float* x, int64_t n, float* partial, radmmm_stream_t stream) {
  RADMMM_REQUIRE(x && partial && n > 0, "sumsq: bad arguments");
  RADMMM_REQUIRE(radmmm::aligned16(x), "sumsq: x must be 16B aligned");
  hipLaunchKernelGGL(sumsq_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, static_cast<hipStream_t>(stream), x, (long long)n, partial);
  return radmmm::check_launch("sumsq");
}

// One RAdam update of a flat buffer.  step_size and the N_sma >= 5 switch are computed by the
// host from the step count exactly as radam.py:101-123; wd_lr = weight_decay * lr;
// clip_coef: optional device scalar applied to the gradient (global-norm clip), null = 1.
extern "C" int radmmm_radam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* clip_coef,
                                 float beta1, float beta2, float eps, float step_size, float wd_lr, int use_denom,
                                 radmmm_stream_t stream) {
  RADMMM_REQUIRE(p && g && m && v && n > 0, "radam_step: bad arguments");
  RADMMM_REQUIRE(radmmm::aligned16(p) && radmmm::aligned16(g) && radmmm::aligned16(m) && radmmm::aligned16(v),
                 "radam_step: the flat buffers must be 16B aligned");
  const long long blocks = (n / 4 + 255) / 256 + 1;
  hipLaunchKernelGGL(radam_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p, g, m, v, (long long)n, clip_coef, beta1, beta2, eps, step_size,
                     wd_lr, use_denom);
  return radmmm::check_launch("radam_step");
}

// The device step counter of one optimizer step: step[0] += 1 unless skip[0] (optional) is non-zero.  One call per step,
// before the buckets' radmmm_adam_step calls, which read the advanced count.
extern "C" int radmmm_adam_advance(int32_t* step, const int32_t* skip, radmmm_stream_t stream) {
  RADMMM_REQUIRE(step, "adam_advance: bad arguments");
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), step, skip);
  return radmmm::check_launch("adam_advance");
}

// One Adam (decoupled = 0: g += wd * p) or AdamW (decoupled = 1: p *= 1 - lr * wd) update of a flat buffer, torch's
// arithmetic: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),
// t = step[0] (device int32, already advanced for this step).  clip_coef: optional device scalar applied to the gradient.
// skip: optional device int32; non-zero leaves p, m and v untouched, whatever g holds.
extern "C" int radmmm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* clip_coef,
                                const int32_t* step, const int32_t* skip, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int decoupled, radmmm_stream_t stream) {
  RADMMM_REQUIRE(p && g && m && v && step && n > 0, "adam_step: bad arguments");
  RADMMM_REQUIRE(radmmm::aligned16(p) && radmmm::aligned16(g) && radmmm::aligned16(m) && radmmm::aligned16(v),
                 "adam_step: the flat buffers must be 16B aligned");
  const long long blocks = (n / 4 + 255) / 256 + 1;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p, g, m, v, (long long)n, clip_coef, step, skip, lr, beta1, beta2, eps,
                     weight_decay, decoupled);
  return radmmm::check_launch("adam_step");
}
