// composer_cols.hpp -- the view of a composer's nine columns that the kernels take by value (composer.hpp) and the host's
// column store hands out (owners.hpp).  Needs the HIP runtime's uint4 and nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pg {

struct ComposerCols {
    uint4 *q[5];
    uint64_t *w[3];
    uint4 *vars;
};

}  // namespace pg
