// radmmm_voc_conv_f16: one dilated Conv1d(C, C, k, dilation d, padding "same") of a HiFi-GAN resblock on the f16 matrix
// cores, channels-last rows [B*T][ld], the leaky-relu of its operand fused into the load (include/radmmm_hip.h has the
// contract, DESIGN.md 4.16 the measurements).
//
// Geometry.  A workgroup (4 waves) owns TM = 128 * MI frames of ONE item and all C output columns.  It reads the frames
// t0 - reach .. t0 + TM + reach of X once, applies in_scale, the leaky-relu, the fp16 clamp and the length mask, and keeps
// that tile as fp16 in LDS ([TM + 2 reach][C + 8] halves; the 16-byte pad makes the row pitch an odd number of 16-byte
// slots, so the 32 rows of a fragment read start in distinct slots).  Rows before the item's first frame, at or past its
// length, are zeros in LDS and are never read from memory.  Every tap is then a row shift inside that tile: the operand
// is converted once and reused taps * C / 32 times.  The weights stream from L2: the (tap, 32-deep k block) pairs form one
// sequence, a step stages G of them ([G][C rows][32 halves]) through registers into LDS -- the loads of step s + 1 are
// issued before the MFMAs of step s and stored after them -- so a step's exposed load latency is paid once per
// G * 2 * MI * NTC MFMAs.  Wave w owns rows w * 32 MI .. + 32 MI of the tile and every column tile: MI x NTC accumulators
// of v_mfma_f32_32x32x16_f16.
//     C <= 32:  NTC 1, MI 4 (TM 512), G 4 (four taps a step)      C <= 64:  NTC 2, MI 2 (TM 256), G 4 (two taps a step)
//     C <= 128: NTC 4, MI 1 (TM 128), G 2 (half a tap a step)     C <= 256: NTC 8, MI 1 (TM 128), G 2 (a quarter)
// so a narrow C spends its registers on rows instead of on empty columns, and C <= 128 keeps LDS under 80 KiB and the
// registers under 256: two workgroups per CU, one loading its tile while the other multiplies (measured at C = 128,
// 32 x 800 frames of V1: 23.3 ms with 256-frame tiles and one workgroup per CU, 20.1 ms with 128-frame tiles and two).
// The tile fill and the epilogue issue their loads in batches ahead of the conversions and stores: with one load per
// loop trip each trip paid a memory latency (V1 at 32 x 800: 110 ms before, 73 ms after).  The epilogue stores from the
// accumulators (lane = column: 128-byte runs per row), no atomics, a fixed summation order: two launches give the same
// bits.
#include "common.h"
#include "split_pack.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxReach = 40;            // (taps / 2) * dil: V1 needs 25, k = 7 with d = 12 needs 36
constexpr int kMaxTaps = 11;
constexpr int BK = 32;                   // halves of K per weight block
constexpr int PB = 40;                   // halves per LDS row of a weight step (80 B: r -> 5r mod 16 is a bijection)
constexpr int kLdsLimit = 160 * 1024;

thread_local int g_voc_f16_last_kernel = 0;

struct voc_plan {
  int ntc, mi;        // column tiles of 32, row tiles of 32 per wave
  int g;              // weight blocks per step
  int reach;
  int lds_bytes;
  int grid;
};

template <int NTC, int MI, int G>
__global__ __launch_bounds__(256) void voc_conv_f16_kernel(const radmmm_voc_conv_f16_desc p, const int tiles_per_item,
                                                           const int reach) {
  extern __shared__ __attribute__((aligned(16))) _Float16 sm[];
  constexpr int TM = 128 * MI;
  constexpr int NB = NTC * 32;                      // weight rows per block
  constexpr int BCH = G * NB * 4 / 256;             // 16-byte chunks per thread and step
  static_assert(G * NB * 4 % 256 == 0, "a step's chunks divide among the threads");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / tiles_per_item, tile = blockIdx.x - b * tiles_per_item;
  const int t0 = tile * TM;
  const int C = p.C, T = p.T;
  int len = p.lens ? p.lens[b] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  const long long row0 = (long long)b * T;
  const int lc = lane & 31, lh = lane >> 5;

  if (t0 >= len) {                                  // the whole tile lies at or past the length: zeros, nothing read
    const int rows = T - t0 < TM ? T - t0 : TM;
    for (int idx = tid; idx < rows * C; idx += 256) {
      const int rl = idx / C, n = idx - rl * C;
      const long long r = row0 + t0 + rl;
      p.Y[r * p.ldy + n] = 0.f;
      if (p.Y2) {
        float* y2 = p.Y2 + r * p.ldy2 + n;
        *y2 = p.y2_accum ? __fadd_rn(*y2, 0.f) : 0.f;
      }
    }
    return;
  }

  const int RA = TM + 2 * reach, PA = C + 8;
  _Float16* As = sm;
  _Float16* Bs = sm + RA * PA;                      // [G][NB][PB]

  // ---- weight steps: blocks f = tap * KB + kb, G per step -> [NB rows][32 halves] each; rows >= C, k >= C and blocks
  // past the last are zeros
  const int KB = (C + BK - 1) / BK;
  const int nblocks = p.taps * KB;
  const int nsteps = (nblocks + G - 1) / G;
  u32x4 breg[BCH];
  auto load_b = [&](int step) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int q = tid + 256 * i;
      const int g = q / (NB * 4), rem = q - g * (NB * 4);
      const int f = step * G + g;
      const int tap = f / KB, kb = f - tap * KB;
      const int n = rem >> 2, k = kb * BK + (rem & 3) * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (f < nblocks && n < C && k < C)
        v = *reinterpret_cast<const u32x4*>(static_cast<const _Float16*>(p.Wh) + ((long long)tap * C + n) * p.ldw + k);
      breg[i] = v;
    }
  };
  auto store_b = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int q = tid + 256 * i;                  // (g * NB + n) * 4 + chunk
      *reinterpret_cast<u32x4*>(Bs + (q >> 2) * PB + (q & 3) * 8) = breg[i];
    }
  };
  load_b(0);

  // ---- the operand tile: h(lrelu(in_scale * x)) inside [0, len), zeros outside.  FU chunks of 8 columns per thread and
  // round, all their loads issued before the first is converted: a round costs one memory latency, not FU
  {
    constexpr int FU = 8;
    const int cpr = C >> 3, total = RA * cpr;
    const float sc = p.in_scale, slope = p.in_slope;
    for (int base = 0; base < total; base += 256 * FU) {
      float4 u[FU], w[FU];
      bool live[FU];
#pragma unroll
      for (int r = 0; r < FU; ++r) {
        const int idx = base + 256 * r + tid;
        const int rl = idx / cpr, ck = idx - rl * cpr;
        const int t = t0 - reach + rl;
        live[r] = idx < total && t >= 0 && t < len;
        u[r] = w[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live[r]) {
          const float4* src = reinterpret_cast<const float4*>(p.X + (row0 + t) * p.ldx + ck * 8);
          u[r] = src[0];
          w[r] = src[1];
        }
      }
#pragma unroll
      for (int r = 0; r < FU; ++r) {
        const int idx = base + 256 * r + tid;
        if (idx >= total) continue;
        const int rl = idx / cpr, ck = idx - rl * cpr;
        const float x[8] = {u[r].x, u[r].y, u[r].z, u[r].w, w[r].x, w[r].y, w[r].z, w[r].w};
        f16x8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = __fmul_rn(x[e], sc);
          v = v >= 0.f ? v : __fmul_rn(slope, v);
          h[e] = live[r] ? (_Float16)radmmm::clamp_f16(v) : (_Float16)0.f;
        }
        *reinterpret_cast<f16x8*>(As + rl * PA + ck * 8) = h;
      }
    }
  }
  store_b();
  __syncthreads();

  f32x16 acc[MI][NTC];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NTC; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int a_row = wave * 32 * MI + lc + reach;    // LDS row of this lane's output row at shift 0 (tile i adds 32 i)
  for (int step = 0; step < nsteps; ++step) {
    const bool more = step + 1 < nsteps;            // uniform
    if (more) load_b(step + 1);                     // in flight during this step's MFMAs
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int f = step * G + g;
      if (f >= nblocks) break;                      // uniform
      const int tap = f / KB, kb = f - tap * KB;
      const int shift = (tap - p.taps / 2) * p.dil;   // |shift| <= reach: a_row + 32 i + shift stays inside [0, RA)
      const _Float16* bb = Bs + (g * NB + lc) * PB + lh * 8;
      const _Float16* ab = As + (a_row + shift) * PA + kb * BK + lh * 8;
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) {
        if (kb * BK + s * 16 < C) {                 // uniform: C is a multiple of 16, not always of 32
          f16x8 a[MI], bf[NTC];
#pragma unroll
          for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const f16x8*>(ab + i * 32 * PA + s * 16);
#pragma unroll
          for (int j = 0; j < NTC; ++j) bf[j] = *reinterpret_cast<const f16x8*>(bb + j * 32 * PB + s * 16);
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NTC; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], bf[j], acc[i][j], 0, 0, 0);
        }
      }
    }
    if (more) {
      __syncthreads();                              // every wave is done with this step's weights
      store_b();
      __syncthreads();
    }
  }

  // ---- epilogue from the accumulators: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  Eight rows at a
  // time: every load of the residual and of Y2 is issued before the first store (Y aliases neither, but the compiler
  // cannot know: in program order a load after a store would wait for its own latency, once per element)
  float bj[NTC];
#pragma unroll
  for (int j = 0; j < NTC; ++j) bj[j] = (j * 32 + lc < C) ? p.bias[j * 32 + lc] : 0.f;
  const float as = p.acc_scale;
  const bool y2_read = p.Y2 && p.y2_accum;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int eh = 0; eh < 2; ++eh) {
      float av[8][NTC], yv[8][NTC];
#pragma unroll
      for (int e8 = 0; e8 < 8; ++e8) {
        const int e = eh * 8 + e8;
        const int t = t0 + wave * 32 * MI + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        const long long r = row0 + t;
#pragma unroll
        for (int j = 0; j < NTC; ++j) {
          const int n = j * 32 + lc;
          av[e8][j] = (p.add && t < len && n < C) ? p.add[r * p.ldadd + n] : 0.f;
          yv[e8][j] = (y2_read && t < T && n < C) ? p.Y2[r * p.ldy2 + n] : 0.f;
        }
      }
#pragma unroll
      for (int e8 = 0; e8 < 8; ++e8) {
        const int e = eh * 8 + e8;
        const int t = t0 + wave * 32 * MI + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (t >= T) continue;
        const bool valid = t < len;
        const long long r = row0 + t;
#pragma unroll
        for (int j = 0; j < NTC; ++j) {
          const int n = j * 32 + lc;
          if (n >= C) continue;
          float v = 0.f;
          if (valid) {
            v = __fadd_rn(__fmul_rn(acc[i][j][e], as), bj[j]);
            if (p.add) v = __fadd_rn(v, av[e8][j]);
          }
          p.Y[r * p.ldy + n] = v;
          if (p.Y2) p.Y2[r * p.ldy2 + n] = p.y2_accum ? __fadd_rn(yv[e8][j], v) : v;
        }
      }
    }
}

// -1: bad arguments; 0: a shape this family does not take (both with the error string set); > 0: the kernel code
int plan_voc_conv_f16(const radmmm_voc_conv_f16_desc* d, voc_plan* pl) {
  RADMMM_REQUIRE(d, "voc_conv_f16: null descriptor");
  RADMMM_REQUIRE(d->X && d->Wh && d->Y && d->bias, "voc_conv_f16: null pointer");
  RADMMM_REQUIRE(d->B > 0 && d->T > 0 && d->C > 0 && d->taps > 0 && d->dil > 0 && (long long)d->B * d->T <= 0x7fffffffLL,
                 "voc_conv_f16: bad dims (B=%d T=%d C=%d taps=%d dil=%d)", d->B, d->T, d->C, d->taps, d->dil);
  RADMMM_REQUIRE(d->ldx >= d->C && d->ldx % 4 == 0 && d->ldw >= d->C && d->ldw % 8 == 0 && d->ldy >= d->C &&
                     (!d->add || d->ldadd >= d->C) && (!d->Y2 || d->ldy2 >= d->C),
                 "voc_conv_f16: bad pitches (C=%d ldx=%d ldw=%d ldy=%d ldadd=%d ldy2=%d; ldx %% 4 == 0, ldw %% 8 == 0)", d->C,
                 d->ldx, d->ldw, d->ldy, d->ldadd, d->ldy2);
  RADMMM_REQUIRE(radmmm::aligned16(d->X) && radmmm::aligned16(d->Wh), "voc_conv_f16: X / Wh must be 16B aligned");
  RADMMM_REQUIRE(d->Y != d->X && d->Y != d->add && d->Y != d->Y2, "voc_conv_f16: Y must alias neither X, add nor Y2");
  const int C = d->C;
  if (C % 16 || C < 16 || C > 256) {
    radmmm::set_error("voc_conv_f16: C=%d not taken (a multiple of 16 in 16 .. 256)", C);
    return 0;
  }
  if (d->taps % 2 == 0 || d->taps > kMaxTaps) {
    radmmm::set_error("voc_conv_f16: taps=%d not taken (odd, at most %d)", d->taps, kMaxTaps);
    return 0;
  }
  const int reach = (d->taps / 2) * d->dil;
  if (reach > kMaxReach) {
    radmmm::set_error("voc_conv_f16: reach (taps / 2) * dil = %d not taken (at most %d)", reach, kMaxReach);
    return 0;
  }
  pl->ntc = C <= 32 ? 1 : C <= 64 ? 2 : C <= 128 ? 4 : 8;
  pl->mi = pl->ntc == 1 ? 4 : pl->ntc == 2 ? 2 : 1;
  pl->g = pl->ntc <= 2 ? 4 : 2;
  pl->reach = reach;
  const int TM = 128 * pl->mi;
  pl->lds_bytes = ((TM + 2 * reach) * (C + 8) + pl->g * pl->ntc * 32 * PB) * 2;
  const long long grid = (long long)d->B * ((d->T + TM - 1) / TM);
  if (pl->lds_bytes > kLdsLimit || grid > 0x7fffffffLL) {   // cannot happen inside the limits above; kept as the last word
    radmmm::set_error("voc_conv_f16: shape not taken (%d bytes of LDS, %lld workgroups)", pl->lds_bytes, grid);
    return 0;
  }
  pl->grid = (int)grid;
  return RADMMM_VOC_F16_KERNEL_CODE(pl->ntc, pl->mi);
}

template <int NTC, int MI, int G>
int launch(const radmmm_voc_conv_f16_desc& d, const voc_plan& pl, hipStream_t stream) {
  static int once = [] {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(voc_conv_f16_kernel<NTC, MI, G>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
    if (e != hipSuccess) {
      radmmm::set_error("hipFuncSetAttribute: %s", hipGetErrorString(e));
      return -2;
    }
    return 0;
  }();
  if (once) return once;
  const int tiles = (d.T + 128 * MI - 1) / (128 * MI);
  hipLaunchKernelGGL((voc_conv_f16_kernel<NTC, MI, G>), dim3(pl.grid), dim3(256), pl.lds_bytes, stream, d, tiles, pl.reach);
  return radmmm::check_launch("voc_conv_f16");
}

}  // namespace

extern "C" int32_t radmmm_voc_conv_f16_plan(const radmmm_voc_conv_f16_desc* d) {
  voc_plan pl;
  return plan_voc_conv_f16(d, &pl);
}

extern "C" int32_t radmmm_voc_conv_f16_last_kernel(void) { return g_voc_f16_last_kernel; }

extern "C" int32_t radmmm_voc_conv_f16(const radmmm_voc_conv_f16_desc* d, radmmm_stream_t stream) {
  voc_plan pl;
  const int code = plan_voc_conv_f16(d, &pl);
  if (code <= 0) return -1;                          // refused, or a shape the plan does not take: no kernel runs
  g_voc_f16_last_kernel = code;
  switch (pl.ntc) {
    case 1: return launch<1, 4, 4>(*d, pl, radmmm::ST(stream));
    case 2: return launch<2, 2, 4>(*d, pl, radmmm::ST(stream));
    case 4: return launch<4, 1, 2>(*d, pl, radmmm::ST(stream));
    default: return launch<8, 1, 2>(*d, pl, radmmm::ST(stream));
  }
}
