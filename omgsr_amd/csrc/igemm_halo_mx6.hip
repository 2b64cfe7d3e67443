// fp6 instantiations of the halo-tile kernel body (igemm_halo_body.hip.h, MX = MX_FP6; round 5): fp16 chunks followed by correction chunks of
// fp6 (e2m3) codes with per-32-channel E8M0 scales taken from the data (OMGSR_EL_MX6 operand + weight packed the same way): the f8f6f4 MFMA
// in its 8-pass form, 1.5x the plain fp16 matrix-pipe time per layer where the fp8 form (igemm_halo_mx.hip) takes 2x. Spatial forms (nine taps, and the four-tap phase form of the up-sampling convs, whose operand igemm_halo_out6.hip / the cast kernel writes).
#include "igemm_halo_body.hip.h"

namespace omgsr {
int igemm_halo_launch_multi_mx6(const void* halo_multi, unsigned blocks, hipStream_t st) {
    const HaloJob j = halo_job(halo_multi, blocks, st);
    return halo_mx_run<MX_FP6>(j, j.m->p[0].upsample != 0, j.m->g[0].cc1 > 0);
}
// g: after halo_geo, spatial form (g.flat == 0)
int igemm_halo_launch_mx6(const omgsr_igemm_args& a, const IgemmGeo& g, hipStream_t st) {
    return halo_mx_run<MX_FP6>(halo_job(a, g, st), a.upsample != 0, false);
}
}  // namespace omgsr
