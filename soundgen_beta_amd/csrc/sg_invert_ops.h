// sg_invert_ops.h — the operator pair (A, A+) of sg_invert.hip as launch sequences, for the
// features built between the two (sg_stretch.hip). Internal; defined in sg_invert.hip beside the
// kernels they launch, so that there is one A and one A+ in the library.
//
// A spectrum has bins + 1 rows and is laid out one sound after the other from cell 0 of d_X, the
// windowed frames likewise from cell 0 of d_ws: sound c of [c0, c1) starts at the sum of
// frames(c') (bins + 1), and frames(c') wl, over the sounds c' before it. A sound with
// lengths[c] < wl (or <= 1) has no frames; A+ then leaves lengths[c] zeros.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "sg_launch.h"
#include "sg_spectrogram.h"

namespace sg {

// A of the sounds as they are (no normalisation: the path of the Griffin-Lim iteration)
template <typename T>
void inv_forward_launch(const SpgSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t c0,
                        int64_t c1, double2* d_X, DevBuf& db, hipStream_t s);
// A+: lengths[c] doubles to d_out + out_off[c]. Stamps clk with sg_invert's stages 3 (inverse
// frames) and 4 (overlap-add).
void inv_synthesis_launch(const SpgSetup& S, const double2* d_X, const int64_t* out_off, const int64_t* lengths,
                          int64_t c0, int64_t c1, double* d_ws, double* d_out, DevBuf& db, StageClock& clk, hipStream_t s);
// consecutive sounds whose needs (bytes) fit the cap; at least one sound a chunk
std::vector<int64_t> inv_chunk_ends(const std::vector<int64_t>& need, int64_t cap);

}  // namespace sg
