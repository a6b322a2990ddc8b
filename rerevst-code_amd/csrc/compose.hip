// compose.hip — librerevst_compose.so: the kernels of the compositing stage behind the delivery stage (include/rerevst_hip.h "Compositing"),
// gfx950, one translation unit and so one code object:
//   compose_k.h    composite_k<MATTE>        strength, matte and colour mix of the stylized frame with its source, one instantiation per matte kind
// and its launch entry.  compose.h is all the main library sees of it; it links this one.  (A library of its own beside librerevst_stages.so
// so that the kernel sets of the other two stay what their ledgers pin.)
#include "compose_k.h"

extern "C" int rrv_compose_launch(const ComposeP* p, int form, void* stream) {
    if (!p || form < 0 || form >= CM_FORMS || !p->P || !p->S || !p->out || p->B < 1 || p->B > CM_B_MAX || p->frame_px < 1) return (int)hipErrorInvalidValue;
    if ((form != CM_NONE) != (p->matte != nullptr) || (form != CM_NONE && p->matte_frames != 1 && p->matte_frames != p->B)) return (int)hipErrorInvalidValue;
    if (p->keep != CK_NONE && p->keep != CK_COLOUR && p->keep != CK_LUMA) return (int)hipErrorInvalidValue;
    ComposeP q = *p;
    q.n_px = (size_t)q.B * q.frame_px;
    const unsigned grid = compose_grid(q.n_px);
    const size_t step = (size_t)grid * 1024;
    q.step_q = step / q.frame_px; q.step_r = step % q.frame_px;
    auto aligned = [](const void* a, size_t to) { return ((uintptr_t)a & (to - 1)) == 0; };
    q.vec = aligned(q.P, 16) && aligned(q.S, 16) && aligned(q.out, 16);
    q.mvec = form != CM_NONE && aligned(q.matte, form == CM_F32 ? 16 : 4) && (q.B == 1 || q.matte_frames == q.B || q.frame_px % 4 == 0);
    static void (*const k[CM_FORMS])(ComposeP) = {composite_k<CM_NONE>, composite_k<CM_F32>, composite_k<CM_U8>};
    hipLaunchKernelGGL(k[form], dim3(grid), dim3(256), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}
