// Halo-tile kernel instantiations whose epilogue writes the fp6 operand form (OMGSR_EL_MX6, omgsr_igemm_args.out_mx = 6) and nothing else: the
// ResnetBlock conv2 in front of an up-sampler, whose only consumer is the up-sampler's phase-form conv (round 5). Two operand forms - plain /
// two-term-split fp16 (the decoder's single layers) and fp6 corrections (MX = 6) - as single launches and launch groups; spatial nine-tap form,
// fp16 compute type, no fused statistics (out_mx excludes gn_partial). A translation unit of its own: as a run-time option of the shared
// epilogue the cooperative store cost every kernel 600+ bytes of scratch (profiles/r05_experiments.md).
#include "igemm_halo_body.hip.h"

namespace omgsr {
// `mx6`: the operand carries fp6 correction chunks
static int out6_run(const HaloJob& j, const bool mx6) {
    return mx6 ? halo_run<f16_t, COLS_128, 9, MX_FP6, FLAT_OFF, GNF_OFF, OUT6_ON>(j) : halo_run<f16_t, COLS_128, 9, MX_NONE, FLAT_OFF, GNF_OFF, OUT6_ON>(j);
}
// what these instantiations can run (omgsr_igemm_out_mx6_ok: the host asks before it requests out_mx = 6)
bool igemm_halo_out6_ok(const omgsr_igemm_args& a) {
    return compute_dtype() == 1 && a.R == 3 && a.S == 3 && a.stride == 1 && !a.upsample && !a.gn_scale_shift && !a.gn_partial && a.Cout > 32 && (a.Cout & 63) == 0 &&
           (a.mx_chunks16 == 0 || a.mx_fmt == 6);          // (never FLAT: halo_flat_eligible() refuses out_mx = 6 problems)
}
int igemm_halo_out6_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st) {
    halo_geo(a, g, false);
    if (g.flat) return OMGSR_E_SHAPE;
    return out6_run(halo_job(a, g, st), a.mx_chunks16 > 0);
}
int igemm_halo_out6_launch_multi(const void* halo_multi, unsigned blocks, hipStream_t st) {
    const HaloJob j = halo_job(halo_multi, blocks, st);
    return out6_run(j, j.m->p[0].mx_chunks16 > 0);
}
}  // namespace omgsr
