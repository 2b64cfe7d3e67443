// GNF instantiations of the halo-tile kernel (igemm_halo_body.hip.h): GroupNorm apply (+ SiLU) as the conv's patch producer. Their own
// translation unit: the in-place transform adds ~60 VALU instructions per piece to a loop that lives at 244 registers, and hipcc compiles
// the files in parallel.
#include "igemm_halo_body.hip.h"

namespace omgsr {
static int gn_run(const HaloJob& j, const bool narrow) {
    if (narrow) OMGSR_DISPATCH_T(return halo_run<T, COLS_32, 9, MX_NONE, FLAT_OFF, GNF_ON>(j));
    OMGSR_DISPATCH_T(return halo_run<T, COLS_128, 9, MX_NONE, FLAT_OFF, GNF_ON>(j));
}

// what the fused form can run (the dispatcher adds the halo kernel's own preconditions and tile-count policy: igemm.hip)
bool igemm_halo_gn_geometry_ok(const omgsr_igemm_args& a) {
    return a.in_el == OMGSR_EL_16 && a.R == 3 && a.S == 3 && a.stride == 1 && !a.upsample && a.in_ld == 0 && !a.in_split && !a.w_split && a.mx_chunks16 == 0 &&
           (a.Cin % 32) == 0 && a.Cin <= GN_MAX_CIN && a.batch == 1 && a.weight_cm != nullptr;
}

int igemm_halo_gn_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st) {
    const bool narrow = halo_geo(a, g, false);
    if (g.flat || a.gn_nimg <= 0) return OMGSR_E_SHAPE;
    return gn_run(halo_job(a, g, st), narrow);
}

int igemm_halo_gn_launch_multi(const void* halo_multi, const unsigned blocks, const bool narrow, hipStream_t st) {
    return gn_run(halo_job(halo_multi, blocks, st), narrow);
}
}  // namespace omgsr
