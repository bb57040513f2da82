// Multi-row GEMV instantiations for __half weights (see gemv_rows.hip, gemv_rows_launch.h).
#include "gemv_rows_launch.h"

namespace llmi {
namespace gemv_detail {
template int rows_launch_epi<__half>(const GemvRowsArgs& p, int grid, hipStream_t s);
}  // namespace gemv_detail
}  // namespace llmi
