// fp16 instantiations of the one-problem-per-grid halo-tile kernel (igemm_halo_body.hip.h); see igemm_halo.hip.
#include "igemm_halo_body.hip.h"

namespace omgsr {
int igemm_halo_launch_f16(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, const bool phase, const bool narrow) {
    using T = f16_t;
    const dim3 grid = halo_grid(g, phase), block(256);
    static const char* var = getenv("OMGSR_HALO_VARIANT");     // A/B runs: "0" = LDS-DMA issued in front of the step's MFMAs
    if (phase) return launch_lds<halo_one<T, COLS_128, 4>>(grid, block, LDS_BYTES, st, a, g);
    if (var && var[0] == '0' && !narrow) return launch_lds<igemm_halo_kernel<T, 5, false>>(grid, block, LDS_BYTES, st, a, g);      // (one-problem kernel only)
    if (narrow) return launch_lds<halo_one<T, COLS_32, 9>>(grid, block, LDS_BYTES, st, a, g);
    return launch_lds<halo_one<T, COLS_128, 9>>(grid, block, LDS_BYTES, st, a, g);
}
}  // namespace omgsr
