// stages.hip — librerevst_stages.so: the kernels of the three frame stages around the network (include/rerevst_hip.h "Scaling", "Output
// size", "Guided delivery"), gfx950, one translation unit and so one code object:
//   resample_k.h   resample_k<IN>            the antialiased resampler in front of the first kernel, one instantiation per input form
//   deliver_k.h    deliver_k<OUT>            the output-side resampler behind the last kernel, one instantiation per output form
//   guided_k.h     gf_coeff_k, gf_apply_k    the guided delivery stage
// and their launch entries.  resample.h, deliver.h and guided.h are all the main library sees of them; it links this one.
#include "resample_k.h"
#include "deliver_k.h"
#include "guided_k.h"

// Queues `k` over `grid` workgroups of 256 threads with `lds` bytes of dynamic LDS.  More than 64 KB of it needs the attribute on the current
// device (lds_max: the most any launch of `k` asks for); set at every launch (cheap), so no state is shared between devices or threads.
template <typename P>
static hipError_t launch_stage(void (*k)(P), unsigned grid, size_t lds, size_t lds_max, const P& p, void* stream) {
    const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
    return hipGetLastError();
}

extern "C" int rrv_scale_launch(const ResampleP* p, int form, void* stream) {
    if (!p || form < 0 || form >= IN_FORMS || p->rows < 1 || p->rows > RS_ROWS_MAX || p->B < 1 || p->tiles_x < 1 || p->tiles_y < 1) return (int)hipErrorInvalidValue;
    static void (*const k[IN_FORMS])(ResampleP) = {resample_k<IN_U8_HWC>,   resample_k<IN_U8_CHW>,   resample_k<IN_F32_HWC>,     resample_k<IN_F32_CHW>,
                                                    resample_k<IN_YUV_I420>, resample_k<IN_YUV_NV12>, resample_k<IN_YUV_I420_16>, resample_k<IN_YUV_P016>};
    return (int)launch_stage(k[form], (unsigned)p->tiles_x * p->tiles_y * p->B, resample_lds_bytes(p->rows), resample_lds_bytes(RS_ROWS_MAX), *p, stream);
}

extern "C" int rrv_deliver_launch(const DeliverP* p, int form, void* stream) {
    if (!p || form < 0 || form >= DL_FORMS || p->rows < 1 || p->rows > RS_ROWS_MAX || p->B < 1 || p->tiles_x < 1 || p->tiles_y < 1) return (int)hipErrorInvalidValue;
    if (p->tiles_x != (p->DW + RS_TW - 1) / RS_TW || p->tiles_y != (p->DH + RS_TH - 1) / RS_TH) return (int)hipErrorInvalidValue;      // (the kernel trusts them)
    static void (*const k[DL_FORMS])(DeliverP) = {deliver_k<DL_F32_HWC>, deliver_k<DL_F32_CHW>, deliver_k<DL_U8_HWC>, deliver_k<DL_U8_CHW>, deliver_k<DL_YUV8>, deliver_k<DL_YUV16>};
    return (int)launch_stage(k[form], (unsigned)p->tiles_x * p->tiles_y * p->B, deliver_lds_bytes(p->rows), deliver_lds_bytes(RS_ROWS_MAX), *p, stream);
}

extern "C" int rrv_guided_launch(const GuidedP* p, void* stream) {
    if (!p || !p->P || !p->xlo || !p->xhi || !p->ab || !p->q) return (int)hipErrorInvalidValue;
    if (p->B < 1 || p->H < 1 || p->W < 1 || p->DH < p->H || p->DW < p->W || p->r < 1 || p->r > GF_R_MAX) return (int)hipErrorInvalidValue;
    if (p->tw != 64 && p->tw != 32 && p->tw != 16 && p->tw != 8) return (int)hipErrorInvalidValue;
    // the kernel stages what p.sy x p.sx holds and no more; smaller than a tile's span would drop taps, so the sizes are the bound's or refused
    if (p->sy != guided_span(p->H, p->DH, GF_AT_H) || p->sx != guided_span(p->W, p->DW, p->tw)) return (int)hipErrorInvalidValue;
    const size_t lds_a = guided_apply_lds_bytes(p->r, p->sy, p->sx);
    if (lds_a > GF_LDS_MAX) return (int)hipErrorInvalidValue;
    const unsigned ct = (unsigned)((p->W + GF_CT_W - 1) / GF_CT_W) * (unsigned)((p->H + GF_CT_H - 1) / GF_CT_H) * (unsigned)p->B;
    const hipError_t e = launch_stage(gf_coeff_k, ct, guided_coeff_lds_bytes(p->r), guided_coeff_lds_bytes(GF_R_MAX), *p, stream);
    if (e != hipSuccess) return (int)e;
    const unsigned at = (unsigned)((p->DW + p->tw - 1) / p->tw) * (unsigned)((p->DH + GF_AT_H - 1) / GF_AT_H) * (unsigned)p->B;
    return (int)launch_stage(gf_apply_k, at, lds_a, GF_LDS_MAX, *p, stream);
}
