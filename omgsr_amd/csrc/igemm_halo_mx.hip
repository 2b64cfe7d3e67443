// Mixed-precision instantiations of the halo-tile kernel body (igemm_halo_body.hip.h, MX = MX_FP8): fp16 chunks followed by block-scaled
// fp8 chunks (v_mfma_scale_f32_32x32x64_f8f6f4) of an OMGSR_EL_MX operand; fp16 compute type, wide nine-tap shape.
#include "igemm_halo_body.hip.h"

namespace omgsr {
int igemm_halo_launch_multi_mx(const void* halo_multi, unsigned blocks, hipStream_t st) {
    const HaloJob j = halo_job(halo_multi, blocks, st);
    if (j.m->p[0].mx_fmt == 6) return igemm_halo_launch_multi_mx6(halo_multi, blocks, st);
    return halo_mx_run<MX_FP8>(j, j.m->p[0].upsample != 0, j.m->g[0].cc1 > 0);
}
int igemm_halo_launch_mx(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st) {
    halo_geo(a, g, a.upsample != 0);
    if (g.flat) return igemm_halo_flat_launch(a, g, st);
    if (a.mx_fmt == 6) return igemm_halo_launch_mx6(a, g, st);
    return halo_mx_run<MX_FP8>(halo_job(a, g, st), a.upsample != 0, false);
}
}  // namespace omgsr
