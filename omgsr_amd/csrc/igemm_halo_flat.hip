// FLAT instantiations of the halo-tile kernel body (igemm_halo_body.hip.h, FLAT != 0): nine taps over the flattened padded map of a
// NARROW image (W <= 45: the tiled VAE's 1/8-resolution tile images), 256 consecutive positions per workgroup. A translation unit of its
// own: the run-time pitch costs the fragment-address table its compile-time geometry, and the spatial instantiations must not pay for it.
#include "igemm_halo_body.hip.h"

namespace omgsr {
// FLAT_22, or FLAT_27: the 27-piece patch (maps 46-80 pixels wide: pitch > 47, i.e. 256 + 2 P + 2 patch rows > 352)
template <int FLAT>
static int flat_run(const HaloJob& j, const bool mx) {
    if (mx) return halo_run<f16_t, COLS_128, 9, MX_FP8, FLAT>(j);
    if (omgsr::compute_dtype() == 1) return halo_run<f16_t, COLS_128, 9, MX_NONE, FLAT>(j);
    return halo_run<bf16_t, COLS_128, 9, MX_NONE, FLAT>(j);
}
// one problem per grid; g comes from halo_geo (g.flat != 0)
int igemm_halo_flat_launch(const omgsr_igemm_args& a, const IgemmGeo& g, hipStream_t st) {
    if (a.mx_chunks16 > 0 && a.mx_fmt == 6) return igemm_halo_flat_launch_mx6(a, g, st);
    const HaloJob j = halo_job(a, g, st);
    return g.flat > FLAT_22_MAX_PITCH ? flat_run<FLAT_27>(j, a.mx_chunks16 > 0) : flat_run<FLAT_22>(j, a.mx_chunks16 > 0);
}
// several problems per launch, at least one of them in the FLAT form (a problem with g.flat == 0 walks its spatial tiles in the same kernel)
int igemm_halo_flat_launch_multi(const void* halo_multi, unsigned blocks, hipStream_t st) {
    const HaloJob j = halo_job(halo_multi, blocks, st);
    const HaloMulti& m = *j.m;
    bool big = false;
    for (int i = 0; i < m.count; ++i) big = big || m.g[i].flat > FLAT_22_MAX_PITCH;         // one kernel per launch: the 27-piece patch serves the narrower problems too
    if (m.p[0].mx_chunks16 > 0 && m.p[0].mx_fmt == 6) return igemm_halo_flat_launch_multi_mx6(halo_multi, blocks, big, st);
    return big ? flat_run<FLAT_27>(j, m.p[0].mx_chunks16 > 0) : flat_run<FLAT_22>(j, m.p[0].mx_chunks16 > 0);
}
}  // namespace omgsr
