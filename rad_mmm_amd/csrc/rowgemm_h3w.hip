// rowgemm_h3w: host side of the split-operand row GEMM (radmmm_rowgemm_h3).  plan_rowgemm_h3 is the ONE decision of what a
// descriptor launches -- validation, buffer extents, narrow (rowgemm_h3.hip) or wide tile, tile height, epilogue kind, kernel
// family (rowgemm_h3w_kernel.h, rowgemm_win.hip, rowgemm_one.hip) -- and the one reader of the family's RADMMM_DEBUG
// switches.  The entry point launches what the plan says; radmmm_rowgemm_h3_plan and radmmm_rowgemm_h3_colsum_rows report it.
// No device code here.
#include <stdlib.h>

#include "common.h"
#include "rowgemm_h3_tiles.h"

extern "C" int radmmm_colsum_final(const float* part, float* out, int nparts, int cols, radmmm_stream_t stream);
extern "C" int radmmm_colsum(const float* X, int ldx, float* out, float* scratch, int rows, int cols, int row_weight, int T,
                             const int32_t* lens, int taps, int dil, int square, radmmm_stream_t stream);

namespace radmmm {

// Workgroup slots a GEMM grid is sized for: the device's CUs, or RADMMM_GEMM_CUS when set (data-parallel runs
// leave a few CUs to RCCL's channel kernels so that an all-reduce landing during a GEMM launch does not push the
// grid into a second round: rad_mmm_amd/ddp.py reserve_collective_cus).  Read once per process.
int gemm_cu_slots() {
  static const int slots = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    if (const char* e = getenv("RADMMM_GEMM_CUS")) {
      const int v = atoi(e);
      if (v >= 32 && v <= n) n = v;
    }
    return n;
  }();
  return slots;
}

namespace {

// The family's experiment / test switches (RADMMM_DEBUG=1 only: debug_env answers nullptr otherwise, without a getenv).
// Three are read once per process, six per launch (tests switch those between cases).
struct h3_switches {
  bool narrow_1x1;       // RADMMM_H3_1X1=128: one-tap launches on the narrow kernel (experiment)
  int mb_max;            // RADMMM_H3W_MB8=0: tile heights 4 .. 7 only (A/B runs)
  bool force_generic;    // RADMMM_DEBUG_EPILOGUE=generic: no direct epilogue (A/B runs, tests)
  int tile;              // RADMMM_H3_TILE=128 / 256: the narrow / the wide tile whatever the grid
  int mb;                // RADMMM_H3W_MB=4 .. 8: this tile height
  bool win, win_xt;      // RADMMM_WIN=0: no shared window under the FP8-cross scheme; RADMMM_WIN_XT=0: none with the extra K segment
  bool one;              // RADMMM_ONE=0: no one-tap kernel under the FP8-cross scheme
  bool slot3;            // RADMMM_SLOT3=0: three-product launches keep rowgemm_h3d
};
int debug_int(const char* name) {                       // a switch's number; -1: not set
  const char* e = debug_env(name);
  return e ? atoi(e) : -1;
}
h3_switches read_h3_switches() {
  static const h3_switches once = [] {
    h3_switches s = {};
    s.narrow_1x1 = debug_int("RADMMM_H3_1X1") == 128;
    s.mb_max = debug_int("RADMMM_H3W_MB8") == 0 ? 7 : 8;
    const char* e = debug_env("RADMMM_DEBUG_EPILOGUE");
    s.force_generic = e && e[0] == 'g';
    return s;
  }();
  h3_switches s = once;
  s.tile = debug_int("RADMMM_H3_TILE");
  s.mb = debug_int("RADMMM_H3W_MB");
  s.win = debug_int("RADMMM_WIN") != 0;
  s.win_xt = debug_int("RADMMM_WIN_XT") != 0;
  s.one = debug_int("RADMMM_ONE") != 0;
  s.slot3 = debug_int("RADMMM_SLOT3") != 0;
  return s;
}

// Row-block count per workgroup.  Cost model fitted to measurements at M = 12 800 and 32 000
// (DESIGN.md §4.2): a workgroup costs (MB + 1.5) units (MFMA work ~ MB, the 256-row B tile and
// the fixed parts ~ 1.5); the grid runs `full` rounds of all CUs plus a tail round which, because the
// chip is power bound, runs faster when few CUs are busy: 0.65 + 0.35 * (tail workgroups / CUs).
int pick_h3w_mb(int M, int N, int slots, int mb_max) {
  const int ntn = (N + BN - 1) / BN;
  int best = 4;
  double best_cost = 1e300;
  // MB = 8 (256-row tiles, 20-36 bytes of scratch per lane) costs what this model says it should on the shape it was
  // measured on (12 800 x 1024: 405 us against 380 us at MB = 7, model 8.77 : 8.22) and is taken where it saves a round
  // of workgroups: N = 1152 (the start conv's data gradient) and N = 1052 (the LSTM's input gradient) fit 50 x 5 = 250
  // workgroups into ONE round instead of 290-500 in two.
  for (int mb = 4; mb <= mb_max; ++mb) {
    const long long wg = (long long)((M + 32 * mb - 1) / (32 * mb)) * ntn;
    const long long full = wg / slots, tail = wg % slots;
    const double rounds = (double)full + (tail ? 0.65 + 0.35 * (double)tail / slots : 0.0);
    const double cost = rounds * (mb + 1.5);
    if (cost <= best_cost + 1e-9) {
      best_cost = cost;
      best = mb;
    }
  }
  return best;
}

// Epilogue kind of a wide-tile launch.  The launches of the flow step (and everything else that fits: even N, no `add`
// input, operands that 32-bit byte offsets can address) take the DIRECT epilogue specialised for the arrays they write
// (EK_*, rowgemm_h3_tiles.h); the rest keeps the fully general LDS-parking epilogue.
int pick_h3w_ek(const radmmm_rowgemm_h3_desc& d, bool force_generic) {
  const radmmm_rowgemm_desc& p = d.base;
  auto a8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; };
  auto a4 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; };
  auto fits = [&](long long ld, int esz) { return ((long long)p.M + 64) * ld * esz < 0x7fffffffLL; };
  // (the pair form of the dact input is decoded by the FP8-cross scheme's direct kernels and by the generic epilogue)
  const bool ok = !force_generic && p.N % 2 == 0 && !p.add && p.ldc % 2 == 0 && a8(p.C) && fits(p.ldc, 4) &&
                  (!p.dact_h || d.nprod == 2) &&
                  (!p.dact || (p.dact_h ? fits(p.lddact_h, 2) : (p.lddact % 2 == 0 && a8(p.dact_src) && fits(p.lddact, 4)))) &&
                  (!p.C2 || (p.ldc2 % 2 == 0 && a8(p.C2) && fits(p.ldc2, 4))) &&
                  (p.n_c2_src <= 0 || (p.ldc2 % 2 == 0 && fits(p.ldc2, 4) && a8(p.c2_src[0]) && a8(p.c2_src[p.n_c2_src > 1 ? 1 : 0]) &&
                                       a8(p.c2_src[p.n_c2_src > 2 ? 2 : 0]))) &&
                  (!p.Ch || (p.ldch % 2 == 0 && a4(p.Ch) && a4(p.Cl) && a4(p.Clo) && fits(p.ldch, 2))) &&
                  (!p.C2h || (p.ldc2h % 2 == 0 && a4(p.C2h) && a4(p.C2l) && fits(p.ldc2h, 2)));
  // (a direct kernel writes its split copies in its own scheme's format: 8-bit cross arrays under nprod 2, fp16 pairs else)
  const bool fmt_ok = (!p.Ch && !p.C2h) || (d.nprod == 2 ? (p.split_fmt == RADMMM_SPLIT_X8A || p.split_fmt == RADMMM_SPLIT_X8B)
                                                          : p.split_fmt == RADMMM_SPLIT_F16);
  if (ok && fmt_ok) {
    if (p.dact) {
      if (!p.C2 && p.Ch && !p.C2h && p.act == RADMMM_ACT_NONE) return EK_DGRAD;
    } else if (p.C2 || p.n_c2_src > 0) {
      if (!p.Ch) return EK_RES;
    } else if (!p.C2h) {
      return p.Ch ? EK_SPLIT : EK_PLAIN;
    }
  }
  return EK_GENERIC;
}

}  // namespace

int plan_rowgemm_h3(const radmmm_rowgemm_h3_desc* d, h3_plan* pl) {
  RADMMM_REQUIRE(d != nullptr, "rowgemm_h3: null descriptor");
  const radmmm_rowgemm_desc& p = d->base;
  RADMMM_REQUIRE(d->Ah && d->Al && d->Bh && d->Bl, "rowgemm_h3: null operand");
  RADMMM_REQUIRE(p.C || p.Ch, "rowgemm_h3: C may be NULL only when the split copy Ch / Cl carries the result");
  RADMMM_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0 && p.taps >= 1 && p.T > 0 && p.M % p.T == 0, "rowgemm_h3: bad dims");
  RADMMM_REQUIRE(p.K % BK == 0, "rowgemm_h3: K=%d must be a multiple of 32", p.K);
  RADMMM_REQUIRE(p.b_layout == 0, "rowgemm_h3: both operands are K-contiguous (use a transposed weight copy)");
  // the framed form (include/radmmm_hip.h): item b, frame t at b * a_item_stride + t * lda_h halves, rows may overlap
  const bool framed = p.a_item_stride != 0;
  RADMMM_REQUIRE(!framed || (p.a_item_stride > 0 && p.a_item_stride % 8 == 0 && p.taps == 1 && !d->extra_tap && !p.a_mask_mode &&
                             d->nprod != 2 && d->lda_h > 0),
                 "rowgemm_h3: a_item_stride (halves, %% 8 == 0) needs one tap, no extra segment, a_mask_mode 0 and nprod 3 or 1");
  RADMMM_REQUIRE(d->lda_h % 8 == 0 && d->ldb_h % 8 == 0 && (framed || d->lda_h >= p.K) && d->ldb_h >= p.K && d->b_tap_stride_h % 8 == 0,
                 "rowgemm_h3: split operands need ld %% 8 == 0 and ld >= K");
  RADMMM_REQUIRE(aligned16(d->Ah) && aligned16(d->Al) && aligned16(d->Bh) && aligned16(d->Bl),
                 "rowgemm_h3: split operands must be 16B aligned");
  RADMMM_REQUIRE(p.sign == 1 || p.sign == -1, "rowgemm_h3: sign must be +-1");
  RADMMM_REQUIRE(!(p.pconv || p.rowscale == 2) || (p.ratio_taps >= 1 && p.ratio_dil >= 1), "rowgemm_h3: ratio_taps/ratio_dil");
  RADMMM_REQUIRE(!p.dact || (p.dact_src != nullptr) != (p.dact_h != nullptr), "rowgemm_h3: dact needs dact_src or the pair dact_h / dact_x");
  RADMMM_REQUIRE(!p.dact_h || (p.dact_x && p.lddact_h % 32 == 0 && p.lddact_h >= p.N && abs(p.dact_x8_exp) <= 16 &&
                               (reinterpret_cast<uintptr_t>(p.dact_h) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.dact_x) & 3) == 0),
                 "rowgemm_h3: dact_h / dact_x: an 8-bit split pair with ld %% 32 == 0");
  RADMMM_REQUIRE(!p.Ch || (p.Cl && p.ldch % 4 == 0 && p.ldch >= ((p.N + 3) & ~3)), "rowgemm_h3: Ch/Cl");
  RADMMM_REQUIRE(p.n_c2_src >= 0 && p.n_c2_src <= 3, "rowgemm_h3: n_c2_src must be 0 .. 3");
  for (int k = 0; k < p.n_c2_src; ++k)
    RADMMM_REQUIRE(p.c2_src[k] && aligned16(p.c2_src[k]), "rowgemm_h3: c2_src[%d] null / not 16-byte aligned", k);
  RADMMM_REQUIRE(p.n_c2_src == 0 || ((p.C2 || p.C2h) && p.ldc2 % 4 == 0 && p.ldc2 >= p.N),
                 "rowgemm_h3: c2_src needs C2 or C2h to receive the sum, and the sources' pitch in ldc2");
  RADMMM_REQUIRE(!p.C2h || (p.C2l && (p.C2 || p.n_c2_src > 0) && p.ldc2h % 4 == 0 && p.ldc2h >= ((p.N + 3) & ~3)), "rowgemm_h3: C2h/C2l");
  RADMMM_REQUIRE(p.split_fmt >= RADMMM_SPLIT_F16 && p.split_fmt <= RADMMM_SPLIT_X8B, "rowgemm_h3: split_fmt");
  RADMMM_REQUIRE(p.split_fmt == RADMMM_SPLIT_F16 || ((!p.Ch || p.ldch % 32 == 0) && (!p.C2h || p.ldc2h % 32 == 0) &&
                                                      abs(p.ch_x8_exp) <= 16 && abs(p.c2h_x8_exp) <= 16),
                 "rowgemm_h3: 8-bit split outputs need ld %% 32 == 0 and |x8_exp| <= 16");
  RADMMM_REQUIRE(d->nprod >= 0 && d->nprod <= 3, "rowgemm_h3: nprod");
  RADMMM_REQUIRE(!p.colsum_out || (p.colsum_scratch && !p.add && !p.C2 && !p.n_c2_src), "rowgemm_h3: colsum_out needs colsum_scratch (and no add / C2 input)");
  RADMMM_REQUIRE(d->nprod != 2 || (abs(d->a8_exp) <= 16 && abs(d->b8_exp) <= 16 && d->lda_h % 32 == 0 && d->ldb_h % 32 == 0 &&
                                   d->b_tap_stride_h % 32 == 0),
                 "rowgemm_h3: nprod 2 needs ld %% 32 == 0 and |x8_exp| <= 16");
  RADMMM_REQUIRE(!d->extra_tap || (d->extra_a_rows >= p.M && p.taps >= 1 && !p.a_mask_mode),
                 "rowgemm_h3: the extra K segment needs extra_a_rows >= M (second matrix behind the first) and a_mask_mode 0");
  const int ntaps = p.taps + (d->extra_tap ? 1 : 0);
  const long long a_bytes = framed ? ((long long)(p.M / p.T - 1) * p.a_item_stride + (long long)(p.T - 1) * d->lda_h + p.K) * 2
                                   : ((long long)p.M + (d->extra_tap ? d->extra_a_rows : 0)) * d->lda_h * 2;
  const long long b_bytes = ((long long)(ntaps - 1) * d->b_tap_stride_h + (long long)p.N * d->ldb_h) * 2;
  RADMMM_REQUIRE(a_bytes < 0x7fffffffLL && b_bytes < 0x7fffffffLL, "rowgemm_h3: operand >= 2 GiB");
  pl->a_bytes = (int)a_bytes;
  pl->b_bytes = (int)b_bytes;
  pl->products = d->nprod == 0 ? 3 : d->nprod;
  pl->colsum_rows = 0;
  const h3_switches sw = read_h3_switches();

  // Narrow or wide tile.  Default: the wide-tile kernels, one workgroup per CU.  A small batch does not give them enough
  // tiles (M = 3200: 100 workgroups of the smallest 128 x 256 tile on 256 CUs): below half a round the 128 x 128 kernel, two
  // workgroups per CU, is faster (B = 8, T = 800: 40.0 vs 43.9 ms per step).  The FP8-cross scheme and the extra K segment
  // exist on the wide kernels only.
  const long long wide_wgs = (long long)((p.M + 127) / 128) * ((p.N + 255) / 256);
  if (d->nprod != 2 && !d->extra_tap &&
      (sw.tile == 128 || (sw.tile != 256 && wide_wgs < 128) || (sw.narrow_1x1 && p.taps == 1))) {
    pl->family = RADMMM_H3_FAMILY_NARROW;
    pl->mb = 4;                                        // (its 128 rows; it has one epilogue, reported as kind 0)
    pl->ek = 0;
    return 0;
  }

  int mb = pick_h3w_mb(p.M, p.N, gemm_cu_slots(), sw.mb_max);
  if (sw.mb >= 4 && sw.mb <= 8) mb = sw.mb;
#ifdef RADMMM_QUICK                                    // development builds instantiate one tile height only
  mb = 7;
#endif
  const int ek = pick_h3w_ek(*d, sw.force_generic);
  pl->mb = mb;
  pl->ek = ek;
  if (ek != EK_GENERIC) pl->colsum_rows = (p.M + 32 * mb - 1) / (32 * mb);

  // Kernel family.  rowgemm_h3d (per-tap A tiles) takes everything; two kernels with a cheaper K loop take what they cover:
  //   rowgemm_win  5-tap convs, the A rows of a k slice fetched once for all taps: MB 7 / 8, dilation <= 8, an utterance at
  //                least as long as the tile (T >= 32 MB: at most one boundary per tile), kinds PLAIN / SPLIT / DGRAD; with
  //                the extra K segment DGRAD only
  //   rowgemm_one  1-tap convs without the extra segment on a three-stage A ring
  // Both step through K in pairs of 32 and exist for two product schemes: FP8 cross terms with the direct kinds, and three
  // f16 products for the C-only launches of the tall tiles (PLAIN, MB 7 / 8, no extra segment: the FiLM stacks' convs and
  // their data gradients, the context LSTM's projection).  The 16-bit throughput mode has rowgemm_h3d only.
  // (What the kernels need besides -- M % T == 0, sign +-1, a_mask_mode 0 with the extra segment -- the validation holds.)
  const bool x8 = d->nprod == 2, tall = mb == 7 || mb == 8;
  const bool scheme = (p.K / BK) % 2 == 0 &&
                      (x8 ? ek != EK_GENERIC : pl->products == 3 && sw.slot3 && tall && ek == EK_PLAIN && !d->extra_tap);
  const bool win = scheme && tall && p.taps == WTAPS && p.dil >= 1 && p.dil <= WDMAX && p.T >= 32 * mb && ek != EK_RES &&
                   (!d->extra_tap || ek == EK_DGRAD) && (!x8 || (sw.win && (sw.win_xt || !d->extra_tap)));
  const bool one = scheme && p.taps == 1 && !d->extra_tap && (!x8 || sw.one);
  pl->family = win ? RADMMM_H3_FAMILY_WIN : one ? RADMMM_H3_FAMILY_ONE : RADMMM_H3_FAMILY_H3D;
  return 0;
}

}  // namespace radmmm

extern "C" int radmmm_rowgemm_h3(const radmmm_rowgemm_h3_desc* d, radmmm_stream_t stream) {
  radmmm::h3_plan pl;
  if (const int rc = radmmm::plan_rowgemm_h3(d, &pl)) return rc;
  radmmm::g_h3_last_kernel = RADMMM_H3_KERNEL_CODE(pl.family, pl.products, pl.mb, pl.ek);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  switch (pl.family) {
    case RADMMM_H3_FAMILY_NARROW: rc = radmmm::launch_rowgemm_h3_narrow(*d, pl, s); break;
    case RADMMM_H3_FAMILY_WIN: rc = radmmm::launch_rowgemm_win(*d, pl, s); break;
    case RADMMM_H3_FAMILY_ONE: rc = radmmm::launch_rowgemm_one(*d, pl, s); break;
    default: rc = pl.products == 2 ? radmmm::launch_h3d_pr2(*d, pl, s) : pl.products == 1 ? radmmm::launch_h3d_pr1(*d, pl, s)
                                                                                          : radmmm::launch_h3d_pr3(*d, pl, s);
  }
  // (optional) the column sums of the launch's pre-row-scale values: from the direct epilogue's per-tile partial rows, or, where
  // the kernel leaves none, by radmmm_colsum over C (weights 1 / ratio: the same sum)
  const radmmm_rowgemm_desc& p = d->base;
  if (rc || !p.colsum_out) return rc;
  if (pl.colsum_rows) return radmmm_colsum_final(p.colsum_scratch, p.colsum_out, pl.colsum_rows, p.N, stream);
  RADMMM_REQUIRE(p.C, pl.family == RADMMM_H3_FAMILY_NARROW
                          ? "rowgemm_h3: colsum_out on this kernel sums C afterwards: C must not be NULL"
                          : "rowgemm_h3: colsum_out with the generic epilogue sums C afterwards: C must not be NULL");
  return radmmm_colsum(p.C, p.ldc, p.colsum_out, p.colsum_scratch, p.M, p.N, p.rowscale == 2 ? 2 : (p.rowscale == 1 ? 1 : 0), p.T,
                       p.lens, p.ratio_taps, p.ratio_dil, 0, stream);
}

extern "C" int radmmm_rowgemm_h3_plan(const radmmm_rowgemm_h3_desc* d) {
  radmmm::h3_plan pl;
  if (const int rc = radmmm::plan_rowgemm_h3(d, &pl)) return rc;
  return RADMMM_H3_KERNEL_CODE(pl.family, pl.products, pl.mb, pl.ek);
}

// rows of partial column sums a launch of *d leaves in colsum_scratch when colsum_out is NULL (include/radmmm_hip.h); 0 = this
// descriptor takes a kernel that leaves none (generic epilogue, the narrow kernel): give it colsum_out
extern "C" int radmmm_rowgemm_h3_colsum_rows(const radmmm_rowgemm_h3_desc* d) {
  radmmm::h3_plan pl;
  if (!d || d->base.M <= 0 || d->base.N <= 0 || !d->base.colsum_scratch || radmmm::plan_rowgemm_h3(d, &pl)) return 0;
  return pl.colsum_rows;
}

extern "C" int radmmm_gemm_cu_slots(void) { return radmmm::gemm_cu_slots(); }
