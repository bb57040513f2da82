// Multi-row GEMV instantiations for int8_t weights (see gemv_rows.hip, gemv_rows_launch.h).
#include "gemv_rows_launch.h"

namespace llmi {
namespace gemv_detail {
template int rows_launch_epi<int8_t>(const GemvRowsArgs& p, int grid, hipStream_t s);
}  // namespace gemv_detail
}  // namespace llmi
