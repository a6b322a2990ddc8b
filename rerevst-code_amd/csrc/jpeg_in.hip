// jpeg_in.hip — librerevst_jpeg_in.so: the kernels of the JPEG input stage (include/rerevst_hip.h "JPEG input"), gfx950, one translation unit and
// so one code object:
//   jpeg_dec_k.h  jpeg_marks_k           the restart markers of every frame's scan -> interval starts, checked against the plan
//                 jpeg_huff_k            one lane per (frame, restart interval): entropy-coded bytes -> coefficient blocks
//                 jpeg_planes_k<HS, VS>  coefficient blocks -> 8-bit planes (dequantise, inverse DCT), one instantiation per chroma format
// and their launch entries.  jpeg_dec.h is all the main library sees of it; it links this one.  (A library of its own beside librerevst_jpeg.so,
// as that one stands beside the other companions: the ledger of the JPEG output stage pins that library's kernel set.)
#include "jpeg_dec_k.h"

static bool jpeg_dec_plan_ok(const JpegDecP* p) {
    if (!p || p->B < 1 || p->B > JP_B_MAX || p->H < 1 || p->W < 1 || !p->frames || !p->coef || ((uintptr_t)p->coef & 15)) return false;
    const bool f = (p->hs == 2 && (p->vs == 2 || p->vs == 1)) || (p->hs == 1 && p->vs == 1);
    if (!f || (p->ncomp != 1 && p->ncomp != 3) || (p->ncomp == 1 && p->hs * p->vs != 1) || p->bpm != (p->ncomp == 1 ? 1 : p->hs * p->vs + 2)) return false;
    if (p->mcu_cols != (p->W + 8 * p->hs - 1) / (8 * p->hs) || p->mcu_rows != (p->H + 8 * p->vs - 1) / (8 * p->vs)) return false;
    if (p->mcus != p->mcu_cols * p->mcu_rows || p->blocks != p->mcus * p->bpm) return false;
    if (p->CH != (p->H + p->vs - 1) / p->vs || p->CW != (p->W + p->hs - 1) / p->hs) return false;
    return p->frame_bytes == (size_t)p->H * p->W + 2 * (size_t)p->CH * p->CW;
}

extern "C" int rrv_jpeg_scan_launch(const JpegDecP* p, void* stream) {
    if (!jpeg_dec_plan_ok(p) || !p->streams || !p->status || !p->ivl || p->n_int_max < 1 || p->n_int_max > p->mcus || p->cap < 1) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(p->coef, 0, (size_t)p->B * p->blocks * 128, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(jpeg_marks_k, dim3((unsigned)p->B), dim3(256), 0, (hipStream_t)stream, *p);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(jpeg_huff_k, dim3((unsigned)((p->n_int_max + 63) / 64), (unsigned)p->B), dim3(64), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}

extern "C" int rrv_jpeg_planes_launch(const JpegDecP* p, void* stream) {
    if (!jpeg_dec_plan_ok(p) || !p->planes) return (int)hipErrorInvalidValue;
    const int g = 32 / p->bpm;
    const dim3 grid((unsigned)((p->mcus + g - 1) / g), (unsigned)p->B);
    if (p->hs == 2 && p->vs == 2) hipLaunchKernelGGL((jpeg_planes_k<2, 2>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    else if (p->hs == 2) hipLaunchKernelGGL((jpeg_planes_k<2, 1>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL((jpeg_planes_k<1, 1>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}
