// picture.hip — librerevst_picture.so: the kernels of the line profile (include/rerevst_hip.h "Picture area"), gfx950, one translation unit
// and so one code object:
//   picture_k.h    picture_lines_k<VEC>   B float32 BGR PIXEL frames -> lit pixels per row, and per column and strip of 32 rows
//                  picture_cols_k         the strips of a column summed
// and their launch entry.  picture.h is all the main library sees of them; it links this one.  (A library of its own so that the kernel
// sets of the other six stay what their ledgers pin.)
#include "picture_k.h"

extern "C" int rrv_picture_launch(const PictureP* p, void* stream) {
    if (!p || !p->in || !p->prof || !p->part || p->B < 1 || p->B > PC_B_MAX || p->H < PC_MIN || p->W < PC_MIN || p->threshold < 0 || p->threshold > PC_T_MAX)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)p->B * (unsigned)pc_strips(p->H));
    const bool vec = p->W % 4 == 0 && (reinterpret_cast<uintptr_t>(p->in) & 15u) == 0;      // every row of every frame starts on 16 bytes
    if (vec) hipLaunchKernelGGL(picture_lines_k<1>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(picture_lines_k<0>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    const int e = (int)hipGetLastError();
    if (e != 0) return e;
    hipLaunchKernelGGL(picture_cols_k, dim3((unsigned)p->B * (unsigned)((p->W + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}
