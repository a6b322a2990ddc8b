// shots.hip — librerevst_shots.so: the kernel of the shot signature (include/rerevst_hip.h "Shots"), gfx950, one translation unit and so one
// code object:
//   shots_k.h    shot_sig_k        B float32 BGR PIXEL frames -> a 32-bin luma histogram per cell of a 4 x 4 grid, exact integer arithmetic
// and its launch entry.  shots.h is all the main library sees of it; it links this one.  (A library of its own so that the kernel sets of the
// other five stay what their ledgers pin.)
#include "shots_k.h"

extern "C" int rrv_shots_launch(const ShotsP* p, void* stream) {
    if (!p || !p->in || !p->sig || p->B < 1 || p->B > SG_B_MAX || p->H < SG_MIN || p->W < SG_MIN) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(shot_sig_k, dim3((unsigned)p->B * SG_CELLS), dim3(256), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}
