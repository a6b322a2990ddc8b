// jpeg.hip — librerevst_jpeg.so: the kernels of the JPEG output stage (include/rerevst_hip.h "JPEG output"), gfx950, one translation unit and so
// one code object:
//   jpeg_k.h    jpeg_blocks_k<HS, VS>    float32 frames -> quantised coefficient blocks, one instantiation per chroma format
//               jpeg_entropy_k<WRITE>    one wave per restart interval: its stuffed length (0), its bytes and RST marker (1)
//               jpeg_place_k             interval offsets, the frame's size against cap, header and EOI
// and their launch entries.  jpeg.h is all the main library sees of it; it links this one.  (A library of its own beside the other companions so
// that their kernel sets stay what their ledgers pin.)
#include "jpeg_k.h"

static bool jpeg_plan_ok(const JpegP* p) {
    if (!p || p->B < 1 || p->B > JP_B_MAX || p->H < 1 || p->W < 1 || !p->coef || ((uintptr_t)p->coef & 15)) return false;
    const bool f = (p->hs == 2 && (p->vs == 2 || p->vs == 1)) || (p->hs == 1 && p->vs == 1);
    if (!f || p->bpm != p->hs * p->vs + 2 || p->mcu_cols != (p->W + 8 * p->hs - 1) / (8 * p->hs) || p->mcu_rows != (p->H + 8 * p->vs - 1) / (8 * p->vs)) return false;
    if (p->mcus != p->mcu_cols * p->mcu_rows || p->blocks != p->mcus * p->bpm || p->interval < 1) return false;
    return p->n_int == (p->mcus + p->interval - 1) / p->interval;
}

extern "C" int rrv_jpeg_blocks_launch(const JpegP* p, void* stream) {
    if (!jpeg_plan_ok(p) || !p->in) return (int)hipErrorInvalidValue;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i)
            if (p->q[t][i] < 1) return (int)hipErrorInvalidValue;
    const int g = 32 / p->bpm;
    const dim3 grid((unsigned)((p->mcus + g - 1) / g), (unsigned)p->B);
    if (p->hs == 2 && p->vs == 2) hipLaunchKernelGGL((jpeg_blocks_k<2, 2>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    else if (p->hs == 2) hipLaunchKernelGGL((jpeg_blocks_k<2, 1>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL((jpeg_blocks_k<1, 1>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}

extern "C" int rrv_jpeg_entropy_launch(const JpegP* p, void* stream) {
    if (!jpeg_plan_ok(p) || !p->out || !p->sizes || !p->lens || !p->offs) return (int)hipErrorInvalidValue;
    if (p->header_len < 1 || p->header_len > JP_HEADER_MAX || p->cap < (size_t)p->header_len || jpeg_bound(*p) > 0x7fffffffu) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)p->n_int, (unsigned)p->B);
    hipLaunchKernelGGL(jpeg_entropy_k<0>, grid, dim3(64), 0, (hipStream_t)stream, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(jpeg_place_k, dim3((unsigned)p->B), dim3(256), 0, (hipStream_t)stream, *p);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(jpeg_entropy_k<1>, grid, dim3(64), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}
