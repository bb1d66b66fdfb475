// rowgemm_h3_tiles.h: what the wide-tile split conv GEMM kernels (rowgemm_h3w_kernel.h, rowgemm_win.hip, rowgemm_one.hip) and
// the host planner (rowgemm_h3w.hip plan_rowgemm_h3) both need to know.  Plain constants: no HIP, no device code.
#pragma once

namespace {

constexpr int BN = 256, BK = 32;                 // columns of a workgroup's tile; channels of a K step
constexpr int WTAPS = 5, WDMAX = 8;              // the shared-window kernel: its tap count, its largest dilation

// epilogue kind of a wide-tile kernel (template parameter; the direct kinds are described in rowgemm_h3w_kernel.h)
//   EK_GENERIC  LDS-parking epilogue, every descriptor option
//   EK_PLAIN    C                                   (bias, row factors, activation)
//   EK_SPLIT    C + split copy Ch / Cl (/ Clo)
//   EK_RES      C + C2 (+)= y (+ split copy C2h / C2l)     side input: C2 when accumulating
//   EK_DGRAD    C + split copy, y multiplied by act'(dact_src)   side input: dact_src
enum { EK_GENERIC = 0, EK_PLAIN, EK_SPLIT, EK_RES, EK_DGRAD, EK_COUNT };

}  // namespace
