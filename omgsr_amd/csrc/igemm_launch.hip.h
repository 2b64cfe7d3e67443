// The host functions that one translation unit of the igemm family calls in another: declared here, once, default arguments included.
// Included by igemm.hip (the dispatcher) and by every unit that defines or calls one of them, so a definition that drifts from its
// declaration fails to compile instead of failing to link (or, with a default argument, silently meaning something else).
#pragma once
#include "common.hip.h"
#include "../../include/omgsr_hip.h"
#include "igemm_epilogue.hip.h"

namespace omgsr {
// ---- GEMM-shaped kernels --------------------------------------------------------------------------------------------------------
int igemm_dma_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st);                                    // igemm_dma.hip
bool igemm_p8_wanted(const omgsr_igemm_args& a, const IgemmGeo& g);                                             // igemm_p8.hip
int igemm_p8_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st);
bool igemm_gmx_ok(const omgsr_igemm_args& a);                                                                   // igemm_gmx.hip
int igemm_gmx_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st);
bool mxfp8_gemm_ok(const omgsr_igemm_args& a);                                 // gemm_mxfp8.hip: OMGSR_EL_MXFP8 operand and weight
int mxfp8_gemm_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st);
int mxfp8_gemm_out8_launch(const omgsr_igemm_args& a, IgemmGeo g, unsigned char* out_scale, int64_t out_scale_ld, hipStream_t st);   // gemm_mxfp8_out8.hip
int mxfp8_gemm_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, int count, hipStream_t st, double flops, double bytes);   // gemm_mxfp8_multi.hip
bool mxfp8_gemm_geglu_ok(const omgsr_igemm_args& a);                           // gemm_mxfp8_geglu.hip: the GEGLU form (out_scale NULL: the plain output)
int mxfp8_gemm_geglu_launch(const omgsr_igemm_args& a, IgemmGeo g, unsigned char* out_scale, int64_t out_scale_ld, hipStream_t st, double flops, double bytes);
bool mxfp8_conv_shape_ok(const omgsr_igemm_args& a);                                                            // conv_mxfp8.hip
int mxfp8_conv_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, double flops);
int mxfp8_conv_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, int count, hipStream_t st, double flops);
bool mxfp8_conv_up_shape_ok(const omgsr_igemm_args& a);                                                         // conv_mxfp8_up.hip
int mxfp8_conv_up_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, double flops);
int mxfp8_conv_up_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, int count, hipStream_t st, double flops);
bool mxfp8_conv_deep_shape_ok(const omgsr_igemm_args& a);                                                       // conv_mxfp8_deep.hip
int mxfp8_conv_deep_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, double flops);

// ---- halo-tile kernel: what the dispatcher asks and calls (igemm_halo.hip, igemm_halo_multi.hip) ------------------------------------
int igemm_halo_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, bool phase = false);
int igemm_halo_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, int count, hipStream_t st, bool phase);
int igemm_halo_launch_splitk(const omgsr_igemm_args& a, const IgemmGeo& g0, int splits, hipStream_t st);
int igemm_halo_tiles(const omgsr_igemm_args& a, bool phase = false);
int igemm_halo_flat(const omgsr_igemm_args& a);      // pitch of the FLAT form the halo kernel would use for this problem (narrow maps), 0 = spatial tiles
int igemm_halo_tiles_form(const omgsr_igemm_args& a, int flat);
int igemm_halo_gn_slots(const omgsr_igemm_args& a, bool phase = false);
bool igemm_halo_gn_geometry_ok(const omgsr_igemm_args& a);     // igemm_halo_gn.hip: what the normalising patch producer can run
bool igemm_halo_out6_ok(const omgsr_igemm_args& a);   // igemm_halo_out6.hip: the instantiations whose epilogue writes OMGSR_EL_MX6 can run this problem

// ---- halo-tile kernel: the per-unit launchers igemm_halo.hip / igemm_halo_multi.hip hand a problem or a launch group on to -----------
// One problem: `g` after halo_geo where it is passed by reference, before it where by value. A launch group: `halo_multi` is the HaloMulti
// of igemm_halo_body.hip.h, whose name lives in that header's anonymous namespace (it is part of the group kernels' symbols) and so cannot
// appear in a declaration shared between units: an opaque pointer, cast back once by each launcher; `blocks` = its 8-aligned block total.
int igemm_halo_launch_f16(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, bool phase, bool narrow);      // igemm_halo_f16.hip
int igemm_halo_launch_mx(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st);                                // igemm_halo_mx.hip
int igemm_halo_launch_multi_mx(const void* halo_multi, unsigned blocks, hipStream_t st);
int igemm_halo_launch_mx6(const omgsr_igemm_args& a, const IgemmGeo& g, hipStream_t st);                        // igemm_halo_mx6.hip
int igemm_halo_launch_multi_mx6(const void* halo_multi, unsigned blocks, hipStream_t st);
int igemm_halo_flat_launch(const omgsr_igemm_args& a, const IgemmGeo& g, hipStream_t st);                       // igemm_halo_flat.hip
int igemm_halo_flat_launch_multi(const void* halo_multi, unsigned blocks, hipStream_t st);
int igemm_halo_flat_launch_mx6(const omgsr_igemm_args& a, const IgemmGeo& g, hipStream_t st);                   // igemm_halo_mx6_flat.hip
int igemm_halo_flat_launch_multi_mx6(const void* halo_multi, unsigned blocks, bool big, hipStream_t st);
int igemm_halo_gn_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st);                                // igemm_halo_gn.hip
int igemm_halo_gn_launch_multi(const void* halo_multi, unsigned blocks, bool narrow, hipStream_t st);
int igemm_halo_out6_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st);                              // igemm_halo_out6.hip
int igemm_halo_out6_launch_multi(const void* halo_multi, unsigned blocks, hipStream_t st);
}  // namespace omgsr
