// product scheme 3 of the wide-tile split conv GEMM (rowgemm_h3w_kernel.h): three f16 products hi.hi + hi.lo + lo.hi
#include "rowgemm_h3w_kernel.h"

namespace radmmm {
int launch_h3d_pr3(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream) { return launch_pr<3>(d, pl, stream); }
}  // namespace radmmm
