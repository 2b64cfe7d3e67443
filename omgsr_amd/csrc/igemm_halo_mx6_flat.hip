// fp6 instantiations of the halo-tile kernel body in its FLAT forms (narrow maps: the tiled VAE's tile images at 1/4 and 1/8 resolution);
// see igemm_halo_mx6.hip for the format and igemm_halo_flat.hip for the form.
#include "igemm_halo_body.hip.h"

namespace omgsr {
static int mx6_flat_run(const HaloJob& j, const bool big) {
    return big ? halo_run<f16_t, COLS_128, 9, MX_FP6, FLAT_27>(j) : halo_run<f16_t, COLS_128, 9, MX_FP6, FLAT_22>(j);
}
int igemm_halo_flat_launch_mx6(const omgsr_igemm_args& a, const IgemmGeo& g, hipStream_t st) {
    return mx6_flat_run(halo_job(a, g, st), g.flat > FLAT_22_MAX_PITCH);
}
int igemm_halo_flat_launch_multi_mx6(const void* halo_multi, unsigned blocks, bool big, hipStream_t st) {
    return mx6_flat_run(halo_job(halo_multi, blocks, st), big);
}
}  // namespace omgsr
