// product scheme 1 of the wide-tile split conv GEMM (rowgemm_h3w_kernel.h): fp16 operands, one product (throughput mode)
#include "rowgemm_h3w_kernel.h"

namespace radmmm {
int launch_h3d_pr1(const radmmm_rowgemm_h3_desc& d, const h3_plan& pl, hipStream_t stream) { return launch_pr<1>(d, pl, stream); }
}  // namespace radmmm
