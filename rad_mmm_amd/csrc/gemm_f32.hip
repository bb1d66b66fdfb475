// fp32 MFMA GEMM kernels for the WN conv stack (gfx950 / CDNA4 only).
//
//  rowgemm_f32  : channels-last Conv1d family (forward and data-gradient), taps folded into
//                 the K loop as row-shifted re-reads of the activation matrix.
//  wgrad_f32    : weight gradient (contraction over frames), split-K into slabs.
//
// Both use v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD): a 128x128 workgroup
// tile, 4 waves in a 2x2 grid, each wave a 2x2 grid of 32x32 MFMA tiles (64 accumulator
// registers).  Operand tiles live in LDS k-major ([BK][128] floats) so that the MFMA
// fragment read (lane l: element [k = l>>5][i = l&31]) is one conflict-free ds_read_b32
// whichever way the operand is laid out in global memory; the two global layouts differ
// only in how the tile is staged (transposing 4x ds_write_b32 vs straight ds_write_b128).
// Global->LDS staging goes through registers, double-buffered in LDS: the loads of tile
// i+1 are issued before the MFMA loop of tile i and written to the other buffer after it,
// one barrier per K step.  fp32 MFMA issues once per 64 cycles per SIMD, which leaves
// ample issue room for the staging traffic (see DESIGN.md for the cycle budget).
#include <stdlib.h>

#include "common.h"
#include "rowgemm_epilogue.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDT = 128;                 // LDS row stride (floats); no padding needed, see above
constexpr int TILE = BK * LDT;           // floats per operand tile
constexpr int SMEM_BYTES = 4 * TILE * 4; // 2 operands x 2 buffers = 64 KiB

__device__ __forceinline__ int xcd_remap(int wg, int nt) {
  // Workgroup b is dispatched to XCD b % 8 (observed; speed only).  Give each XCD a
  // contiguous chunk of tile ids so tiles that share an A panel share an L2.
  const int xcd = wg & 7, loc = wg >> 3;
  const int q = nt >> 3, r = nt & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

__device__ __forceinline__ float4 sel4(float4 v, bool ok, int k, int K) {
  v.x = (ok && k + 0 < K) ? v.x : 0.f;
  v.y = (ok && k + 1 < K) ? v.y : 0.f;
  v.z = (ok && k + 2 < K) ? v.z : 0.f;
  v.w = (ok && k + 3 < K) ? v.w : 0.f;
  return v;
}

__device__ __forceinline__ void mfma_step(const float* as, const float* bs, f32x16 (&acc)[2][2]) {
  // as/bs already offset by wave sub-tile + (lane&31) + (lane>>5)*LDT.  Fragments of k-pair
  // kk+1 are read from LDS before the MFMAs of k-pair kk issue, so the LDS latency sits
  // under 4 MFMAs (256 cycles) instead of in front of them.
  float a[2][2], b[2][2];
  a[0][0] = as[0]; a[0][1] = as[32];
  b[0][0] = bs[0]; b[0][1] = bs[32];
#pragma unroll
  for (int kk = 0; kk < BK / 2; ++kk) {
    const int cur = kk & 1, nxt = cur ^ 1;
    if (kk + 1 < BK / 2) {
      a[nxt][0] = as[(kk + 1) * 2 * LDT]; a[nxt][1] = as[(kk + 1) * 2 * LDT + 32];
      b[nxt][0] = bs[(kk + 1) * 2 * LDT]; b[nxt][1] = bs[(kk + 1) * 2 * LDT + 32];
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads ahead of this k-pair's MFMAs
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][0], b[cur][0], acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][0], b[cur][1], acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][1], b[cur][0], acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][1], b[cur][1], acc[1][1], 0, 0, 0);
  }
}

// Write a workgroup's accumulators to LDS as a row-major [128][128] fp32 tile.  MFMA 32x32
// C/D layout: lane l, register e -> column l&31, row (e&3) + 8*(e>>2) + 4*(l>>5).
__device__ __forceinline__ void stage_acc_to_lds(float* smem, const f32x16 (&acc)[2][2], int wm,
                                                 int wn, int lane) {
  float* base = smem + (wm * 64 + 4 * (lane >> 5)) * BN + wn * 64 + (lane & 31);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        base[(mi * 32 + (e & 3) + 8 * (e >> 2)) * BN + ni * 32] = acc[mi][ni][e];
}

// ------------------------------------------------------------------------------------
// rowgemm
// ------------------------------------------------------------------------------------
template <int B_LAYOUT>
__global__ __launch_bounds__(256, 2) void rowgemm_f32_kernel(const radmmm_rowgemm_desc p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;             // [2][BK][LDT]
  float* Bs = smem + 2 * TILE;  // [2][BK][LDT]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (p.N + BN - 1) / BN, ntm = (p.M + BM - 1) / BM;
  const int tile = xcd_remap(blockIdx.x, ntn * ntm);
  const int tm = tile / ntn, tn = tile - tm * ntn;
  const int m0 = tm * BM, n0 = tn * BN;

  const int kpt = (p.K + BK - 1) / BK;  // K steps per tap
  const int nsteps = kpt * p.taps;

  // ---- per-thread staging coordinates -------------------------------------------------
  // A (always [row][k], k contiguous): thread owns row a_row, 16-byte chunks a_kc + 2*i
  const int a_row = tid & 127, a_kc = tid >> 7;
  const int r = m0 + a_row;
  const bool r_ok = r < p.M;
  int t_in = 0, lim = 0;
  const float* a_item_ptr = p.A;   // frame 0 of this thread's item (always valid memory)
  if (r_ok) {
    const int b = r / p.T;
    t_in = r - b * p.T;
    lim = (p.a_mask_mode && p.lens) ? p.lens[b] : p.T;
    a_item_ptr = p.A + (p.a_item_stride ? (long long)b * p.a_item_stride : (long long)b * p.T * p.lda);
  }
  // B layout 0 ([n][k]): same shape as A.  B layout 1 ([k][n]): thread owns 4 n at b_n4*4,
  // k rows b_k0 + 8*i.
  const int b_n4 = tid & 31, b_k0 = tid >> 5;
  const int bn = n0 + a_row;  // layout 0 row
  const bool bn_ok = bn < p.N;

  float4 ra[4], rb[4];

  // Loads only ISSUE here (addresses clamped to valid memory); the validity selects are
  // applied in store_tiles, i.e. after the MFMA loop of the current tile, so that the
  // s_waitcnt for these loads lands behind the MFMAs and not in front of them.
  auto load_tiles = [&](int step) {
    const int tap = step / kpt, kb = step - tap * kpt;
    const int s = p.sign * (tap - p.taps / 2) * p.dil;
    const int ts = t_in + s;
    const bool av = r_ok && ts >= 0 && ts < lim;
    const float* arow = a_item_ptr + (long long)(av ? ts : 0) * p.lda;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = kb * BK + (a_kc + 2 * i) * 4;
      ra[i] = *reinterpret_cast<const float4*>(arow + ((av && k < p.K) ? k : 0));
    }
    const float* bbase = p.B + (long long)tap * p.b_tap_stride;
    if (B_LAYOUT == 0) {
      const float* brow = bbase + (long long)(bn_ok ? bn : 0) * p.ldb;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = kb * BK + (a_kc + 2 * i) * 4;
        rb[i] = *reinterpret_cast<const float4*>(brow + ((bn_ok && k < p.K) ? k : 0));
      }
    } else {
      const int n = n0 + b_n4 * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = kb * BK + b_k0 + 8 * i;
        const bool kv = k < p.K && n < p.N;
        rb[i] = *reinterpret_cast<const float4*>(bbase + (long long)(kv ? k : 0) * p.ldb + (kv ? n : 0));
      }
    }
  };
  auto store_tiles = [&](int step, int buf) {
    const int tap = step / kpt, kb = step - tap * kpt;
    const int ts = t_in + p.sign * (tap - p.taps / 2) * p.dil;
    const bool av = r_ok && ts >= 0 && ts < lim;
    float* as = As + buf * TILE;
    float* bs = Bs + buf * TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kc = (a_kc + 2 * i) * 4;
      const int k = kb * BK + kc;
      const float4 v = sel4(ra[i], av && k < p.K, k, p.K);
      as[(kc + 0) * LDT + a_row] = v.x;
      as[(kc + 1) * LDT + a_row] = v.y;
      as[(kc + 2) * LDT + a_row] = v.z;
      as[(kc + 3) * LDT + a_row] = v.w;
    }
    if (B_LAYOUT == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kc = (a_kc + 2 * i) * 4;
        const int k = kb * BK + kc;
        const float4 v = sel4(rb[i], bn_ok && k < p.K, k, p.K);
        bs[(kc + 0) * LDT + a_row] = v.x;
        bs[(kc + 1) * LDT + a_row] = v.y;
        bs[(kc + 2) * LDT + a_row] = v.z;
        bs[(kc + 3) * LDT + a_row] = v.w;
      }
    } else {
      const int n = n0 + b_n4 * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = kb * BK + b_k0 + 8 * i;
        *reinterpret_cast<float4*>(bs + (b_k0 + 8 * i) * LDT + b_n4 * 4) = sel4(rb[i], k < p.K && n < p.N, n, p.N);
      }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  load_tiles(0);
  store_tiles(0, 0);
  __syncthreads();
  const int frag_off = (lane >> 5) * LDT + (lane & 31);
  for (int step = 0; step < nsteps; ++step) {
    // single basic block: the last iteration re-stages the final tile into the idle buffer
    // instead of branching, so the loads' wait sits behind the MFMAs in every iteration
    const int buf = step & 1;
    const int nxt = step + 1 < nsteps ? step + 1 : step;
    load_tiles(nxt);
    mfma_step(As + buf * TILE + wm * 64 + frag_off, Bs + buf * TILE + wn * 64 + frag_off, acc);
    store_tiles(nxt, buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue --------------------------------------------------------------------------
  // Stage the 128x128 accumulator tile through LDS (free after the K loop; the loop's last
  // barrier has passed) so that global traffic is row-contiguous float4 and the per-row
  // mask/ratio is computed once per 4 outputs.
  stage_acc_to_lds(smem, acc, wm, wn, lane);
  __syncthreads();
  const radmmm::EpilogueCtx ec(p);
  const int c4 = (tid & 31) * 4;
  for (int i = 0; i < 16; ++i) {
    const int rl = i * 8 + (tid >> 5);
    const float4 a4 = *reinterpret_cast<const float4*>(smem + rl * BN + c4);
    radmmm::epilogue_store4(p, ec, m0 + rl, n0 + c4, a4);
  }
}

// ------------------------------------------------------------------------------------
// wgrad: P[split][tap][m][n] = sum_r GY[r][m] * Xm[r + shift(tap)][n]
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void wgrad_f32_kernel(const radmmm_wgrad_desc p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;
  float* Bs = smem + 2 * TILE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntm = (p.Mc + BM - 1) / BM, ntn = (p.Nc + BN - 1) / BN;
  // blockIdx.x -> (tile_n fastest, tile_m, tap, split)
  int id = blockIdx.x;
  const int tn = id % ntn; id /= ntn;
  const int tm = id % ntm; id /= ntm;
  const int tap = id % p.taps;
  const int split = id / p.taps;
  const int m0 = tm * BM, n0 = tn * BN;
  const int shift = (tap - p.taps / 2) * p.dil;

  // rows of this split, in units of BK
  const int steps_total = (p.R + BK - 1) / BK;
  const int steps_per = (steps_total + p.splits - 1) / p.splits;
  const int step_lo = split * steps_per;
  int step_hi = step_lo + steps_per;
  if (step_hi > steps_total) step_hi = steps_total;

  const int c4 = tid & 31, k0 = tid >> 5;  // 4 columns at c4*4, k rows k0 + 8*i
  const int am = m0 + c4 * 4, bn = n0 + c4 * 4;

  float4 ra[4], rb[4];
  auto x_row = [&](int rr, bool& ok) {   // source row of the (shifted, masked) activation operand
    ok = rr < p.R && bn < p.Nc;
    int src = 0;
    if (ok) {
      const int b = rr / p.T;
      const int t = rr - b * p.T + shift;
      const int lim = (p.x_mask_mode && p.lens) ? p.lens[b] : p.T;
      ok = t >= 0 && t < lim;
      src = rr + shift;
    }
    return ok ? src : 0;
  };
  auto load_tiles = [&](int step) {     // issue only; selects happen in store_tiles
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = step * BK + k0 + 8 * i;
      const bool aok = rr < p.R && am < p.Mc;
      ra[i] = *reinterpret_cast<const float4*>(p.GY + (long long)(aok ? rr : 0) * p.ldgy + (aok ? am : 0));
      bool bok;
      const int src = x_row(rr, bok);
      rb[i] = *reinterpret_cast<const float4*>(p.X + (long long)src * p.ldx + (bok ? bn : 0));
    }
  };
  auto store_tiles = [&](int step, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = step * BK + k0 + 8 * i;
      const bool aok = rr < p.R && am < p.Mc;
      bool bok;
      (void)x_row(rr, bok);
      *reinterpret_cast<float4*>(As + buf * TILE + (k0 + 8 * i) * LDT + c4 * 4) = sel4(ra[i], aok, am, p.Mc);
      *reinterpret_cast<float4*>(Bs + buf * TILE + (k0 + 8 * i) * LDT + c4 * 4) = sel4(rb[i], bok, bn, p.Nc);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int frag_off = (lane >> 5) * LDT + (lane & 31);
  if (step_lo < step_hi) {
    load_tiles(step_lo);
    store_tiles(step_lo, 0);
    __syncthreads();
    for (int step = step_lo; step < step_hi; ++step) {
      const int buf = (step - step_lo) & 1;
      const int nxt = step + 1 < step_hi ? step + 1 : step;
      load_tiles(nxt);
      mfma_step(As + buf * TILE + wm * 64 + frag_off, Bs + buf * TILE + wn * 64 + frag_off, acc);
      store_tiles(nxt, buf ^ 1);
      __syncthreads();
    }
  }

  float* P = p.P + (long long)split * p.split_stride + (long long)tap * p.Mc * p.ldp;
  stage_acc_to_lds(smem, acc, wm, wn, lane);
  __syncthreads();
  const bool vec_ok = (p.ldp % 4 == 0) && radmmm::aligned16(p.P) && (p.split_stride % 4 == 0);
  const int col = n0 + c4 * 4;
  for (int i = 0; i < 16; ++i) {
    const int rl = i * 8 + (tid >> 5);
    const int row = m0 + rl;
    if (row >= p.Mc || col >= p.Nc) continue;
    const float4 a4 = *reinterpret_cast<const float4*>(smem + rl * BN + c4 * 4);
    if (vec_ok && col + 3 < p.Nc) {
      *reinterpret_cast<float4*>(P + (long long)row * p.ldp + col) = a4;
    } else {
      const float v[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < p.Nc) P[(long long)row * p.ldp + col + e] = v[e];
    }
  }
}

template <typename K>
int ensure_smem(K kernel) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
  if (e != hipSuccess) {
    radmmm::set_error("hipFuncSetAttribute(max dynamic LDS): %s", hipGetErrorString(e));
    return -2;
  }
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------
// The one decision of the fp32 family: descriptor validation, then which kernel a descriptor takes and with which
// tiling and buffer extents.  Host only -- no HIP call, no operand pointer dereferenced -- so radmmm_rowgemm_f32_plan /
// radmmm_wgrad_f32_plan answer on a machine without a GPU, and the entry points switch on the same result.
// ------------------------------------------------------------------------------------
int radmmm::plan_rowgemm_f32(const radmmm_rowgemm_desc* d, radmmm::f32_plan* pl) {
  RADMMM_REQUIRE(d != nullptr, "rowgemm: null descriptor");
  RADMMM_REQUIRE(d->A && d->B && d->C, "rowgemm: null operand");
  RADMMM_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->taps >= 1 && d->T > 0, "rowgemm: bad dims M=%d N=%d K=%d taps=%d T=%d", d->M, d->N, d->K, d->taps, d->T);
  RADMMM_REQUIRE(d->M % d->T == 0, "rowgemm: M=%d is not a multiple of T=%d", d->M, d->T);
  RADMMM_REQUIRE(d->lda % 4 == 0 && radmmm::aligned16(d->A) && d->a_item_stride % 4 == 0, "rowgemm: A must be 16B aligned with lda %% 4 == 0 (lda=%d)", d->lda);
  RADMMM_REQUIRE(d->a_item_stride != 0 || d->lda >= ((d->K + 3) & ~3), "rowgemm: lda >= roundup4(K) required unless a_item_stride is set (lda=%d K=%d)", d->lda, d->K);
  if (d->b_layout == 0) {
    RADMMM_REQUIRE(d->ldb % 4 == 0 && d->ldb >= ((d->K + 3) & ~3), "rowgemm: B[n][k] needs ldb %% 4 == 0 and ldb >= roundup4(K) (ldb=%d K=%d)", d->ldb, d->K);
  } else {
    RADMMM_REQUIRE(d->b_layout == 1, "rowgemm: b_layout must be 0 or 1");
    RADMMM_REQUIRE(d->ldb % 4 == 0 && d->ldb >= ((d->N + 3) & ~3), "rowgemm: B[k][n] needs ldb %% 4 == 0 and ldb >= roundup4(N) (ldb=%d N=%d)", d->ldb, d->N);
  }
  RADMMM_REQUIRE(radmmm::aligned16(d->B) && d->b_tap_stride % 4 == 0, "rowgemm: B must be 16B aligned, tap stride %% 4 == 0");
  RADMMM_REQUIRE(d->sign == 1 || d->sign == -1, "rowgemm: sign must be +-1");
  RADMMM_REQUIRE(!(d->pconv || d->rowscale == 2) || (d->ratio_taps >= 1 && d->ratio_dil >= 1), "rowgemm: ratio_taps/ratio_dil required with pconv/rowscale=2");
  RADMMM_REQUIRE(!d->dact || d->dact_src, "rowgemm: dact needs dact_src");
  *pl = radmmm::f32_plan{};
  pl->bl = d->b_layout;
  pl->ntn = (d->N + BN - 1) / BN;

  // (1) the flow steps' 160 x 160 channel mix and its data gradient: the whole weight in LDS, no barrier in the K loop
  // (rowgemm_mix.hip).  Scope: N == K == 160, one tap, no mask / ratio / activation / add / second output / split copy;
  // bias optional.  RADMMM_MIX=0 (RADMMM_DEBUG) disables it (A/B runs).
  static const bool mix_off = [] {
    const char* e = radmmm::debug_env("RADMMM_MIX");
    return e && e[0] == '0';
  }();
  constexpr int NK = radmmm::kMixNK;
  if (!mix_off && d->N == NK && d->K == NK && d->taps == 1 && d->a_item_stride == 0 && !d->a_mask_mode && !d->pconv && !d->premask &&
      !d->postmask && !d->add && !d->dact && !d->rowscale && d->act == RADMMM_ACT_NONE && !d->C2 && !d->Ch && !d->C2h &&
      !d->colsum_out && !d->n_c2_src && d->ldc % 4 == 0 && d->lda >= NK && d->ldb >= NK && d->ldc >= NK &&
      radmmm::aligned16(d->C)) {
    pl->family = RADMMM_F32_FAMILY_MIX;
    return 0;
  }

  // (2) 16-row-granular tiling with a VALU-free K loop (rowgemm16_f32.hip): needs K % 16 == 0 and operands < 2 GiB.
  // RADMMM_ROWGEMM_TILE=32 (RADMMM_DEBUG) forces the generic kernels.
  static const bool use32 = [] {
    const char* e = radmmm::debug_env("RADMMM_ROWGEMM_TILE");
    return e && atoi(e) == 32;
  }();
  if (!use32 && d->K % 16 == 0) {
    // tiling choice: minimise (rounds of 512 workgroup slots) x (MFMA rows per workgroup + fixed per-step overhead),
    // i.e. the modelled time of the busiest CU
    static const int kMT[] = {4, 6, 8, 10, 12, 13, 14, 15};
    const int ntn = pl->ntn;
    const int slots = 512;
    double best_cost = 1e300;
    int best_mt = 15, best_rows = 240, best_nmt = (d->M + 239) / 240;
    for (int mt : kMT) {
      const int cap = mt * 16;
      const int nmt_min = (d->M + cap - 1) / cap;
      // try the minimal tile count for this MT and the next few counts that complete a round
      for (int extra = 0; extra < 3; ++extra) {
        int nmt = nmt_min;
        if (extra) {
          const long long wg = (long long)nmt_min * ntn;
          const long long rounds = (wg + slots - 1) / slots + (extra - 1);
          nmt = (int)((rounds * slots) / ntn);
          if (nmt < nmt_min) continue;
        }
        if (nmt > d->M) nmt = d->M;
        const int rows = (d->M + nmt - 1) / nmt;
        if (rows > cap) continue;
        nmt = (d->M + rows - 1) / rows;
        const long long wg = (long long)nmt * ntn;
        const double rounds = (double)((wg + slots - 1) / slots);
        // a partially filled single round costs the same as a full one for the busiest CU, but
        // with < 256 workgroups only one workgroup runs per CU (no sharing of the MFMA pipe)
        const double share = wg <= 256 ? 0.6 : 1.0;
        const double cost = rounds * share * (mt + 1.5);
        if (cost < best_cost - 1e-9) {
          best_cost = cost;
          best_mt = mt;
          best_rows = rows;
          best_nmt = nmt;
        }
      }
    }
    // byte extents of the operands for the buffer descriptors
    // With a_item_stride and a_mask_mode 1 an item may hold more frames than the T that are written (lens[b] > T: the
    // inverse STFT reads F = T + 1 frames per item), so a tap of the LAST item may reach taps/2 * dil frames past T - 1;
    // the descriptor must span them, or that item reads zeros there while every other item reads the frames.  lens lives
    // on the device, so the launcher cannot tell whether the last item is that long and always spans the reach; the
    // kernel still masks every frame at or above lens[b], so the wider extent admits only frames the caller holds.
    const long long items = d->M / d->T;
    const long long reach = (d->a_item_stride && d->a_mask_mode && d->lens) ? (long long)(d->taps / 2) * d->dil : 0;
    const long long a_last = d->a_item_stride ? (items - 1) * d->a_item_stride + (d->T - 1 + reach) * d->lda
                                              : (long long)(d->M - 1) * d->lda;
    const long long a_bytes = (a_last + d->K) * 4;
    // (measured on gfx950: the scalar offset IS part of the hardware range check, so the descriptor
    //  spans the whole operand and invalid elements are flagged through the vector offset alone)
    const long long b_bytes = ((long long)(d->taps - 1) * d->b_tap_stride +
                               (d->b_layout == 0 ? (long long)d->N * d->ldb : (long long)d->K * d->ldb)) * 4;
    if (a_bytes < 0x7fffffffLL && b_bytes < 0x7fffffffLL) {
      pl->family = RADMMM_F32_FAMILY_ROWS16;
      pl->mt = best_mt;
      pl->rows = best_rows;
      pl->nmt = best_nmt;
      pl->a_bytes = (int)a_bytes;
      pl->b_bytes = (int)b_bytes;
      return 0;
    }
  }
  // (3) the generic 128 x 128 kernel
  pl->family = RADMMM_F32_FAMILY_GENERIC;
  return 0;
}

int radmmm::plan_wgrad_f32(const radmmm_wgrad_desc* d, radmmm::f32_plan* pl) {
  RADMMM_REQUIRE(d != nullptr, "wgrad: null descriptor");
  RADMMM_REQUIRE(d->GY && d->X && d->P, "wgrad: null operand");
  RADMMM_REQUIRE(d->R > 0 && d->Mc > 0 && d->Nc > 0 && d->taps >= 1 && d->T > 0 && d->splits >= 1, "wgrad: bad dims");
  RADMMM_REQUIRE(d->R % d->T == 0, "wgrad: R=%d is not a multiple of T=%d", d->R, d->T);
  RADMMM_REQUIRE(d->ldgy % 4 == 0 && d->ldgy >= ((d->Mc + 3) & ~3) && radmmm::aligned16(d->GY), "wgrad: GY alignment (ldgy=%d Mc=%d)", d->ldgy, d->Mc);
  RADMMM_REQUIRE(d->ldx % 4 == 0 && d->ldx >= ((d->Nc + 3) & ~3) && radmmm::aligned16(d->X), "wgrad: X alignment (ldx=%d Nc=%d)", d->ldx, d->Nc);
  RADMMM_REQUIRE(d->ldp >= d->Nc, "wgrad: ldp < Nc");
  *pl = radmmm::f32_plan{};
  pl->family = RADMMM_F32_FAMILY_WGRAD;
  static const bool generic_only = [] {
    const char* e = radmmm::debug_env("RADMMM_ROWGEMM_TILE");
    return e && atoi(e) == 32;
  }();
  // fast path (wgrad16_f32.hip): every K step of 16 frames inside one item, operands < 2 GiB
  constexpr int BK16 = radmmm::kWgrad16BK;
  if (!generic_only && d->T % BK16 == 0 && d->R % BK16 == 0) {
    const long long gy_bytes = (long long)d->R * d->ldgy * 4, x_bytes = (long long)d->R * d->ldx * 4;
    if (gy_bytes < 0x7fffffffLL && x_bytes < 0x7fffffffLL) {
      pl->family = RADMMM_F32_FAMILY_WGRAD16;
      pl->a_bytes = (int)gy_bytes;
      pl->b_bytes = (int)x_bytes;
    }
  }
  return 0;
}

static int plan_code(const radmmm::f32_plan& pl) {
  return RADMMM_F32_KERNEL_CODE(pl.family, pl.bl, pl.mt, pl.rows);
}

extern "C" int radmmm_rowgemm_f32_plan(const radmmm_rowgemm_desc* d) {
  radmmm::f32_plan pl;
  const int rc = radmmm::plan_rowgemm_f32(d, &pl);
  return rc < 0 ? rc : plan_code(pl);
}

extern "C" int radmmm_wgrad_f32_plan(const radmmm_wgrad_desc* d) {
  radmmm::f32_plan pl;
  const int rc = radmmm::plan_wgrad_f32(d, &pl);
  return rc < 0 ? rc : plan_code(pl);
}

extern "C" int radmmm_rowgemm_f32(const radmmm_rowgemm_desc* d, radmmm_stream_t stream) {
  radmmm::f32_plan pl;
  const int rc = radmmm::plan_rowgemm_f32(d, &pl);
  if (rc < 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (pl.family == RADMMM_F32_FAMILY_MIX) return radmmm::launch_rowgemm_mix(*d, pl, s);
  if (pl.family == RADMMM_F32_FAMILY_ROWS16) return radmmm::launch_rowgemm16(*d, pl, s);
  const int ntm = (d->M + BM - 1) / BM;
  if (pl.bl == 0) {
    static int once = ensure_smem(rowgemm_f32_kernel<0>);
    if (once) return once;
    hipLaunchKernelGGL(rowgemm_f32_kernel<0>, dim3(ntm * pl.ntn), dim3(256), SMEM_BYTES, s, *d);
  } else {
    static int once = ensure_smem(rowgemm_f32_kernel<1>);
    if (once) return once;
    hipLaunchKernelGGL(rowgemm_f32_kernel<1>, dim3(ntm * pl.ntn), dim3(256), SMEM_BYTES, s, *d);
  }
  return radmmm::check_launch("rowgemm_f32");
}

extern "C" int radmmm_wgrad_f32(const radmmm_wgrad_desc* d, radmmm_stream_t stream) {
  radmmm::f32_plan pl;
  const int rc = radmmm::plan_wgrad_f32(d, &pl);
  if (rc < 0) return rc;
  if (pl.family == RADMMM_F32_FAMILY_WGRAD16) return radmmm::launch_wgrad16(*d, pl, static_cast<hipStream_t>(stream));
  const int ntm = (d->Mc + BM - 1) / BM, ntn = (d->Nc + BN - 1) / BN;
  static int once = ensure_smem(wgrad_f32_kernel);
  if (once) return once;
  hipLaunchKernelGGL(wgrad_f32_kernel, dim3(ntm * ntn * d->taps * d->splits), dim3(256), SMEM_BYTES,
                     static_cast<hipStream_t>(stream), *d);
  return radmmm::check_launch("wgrad_f32");
}
