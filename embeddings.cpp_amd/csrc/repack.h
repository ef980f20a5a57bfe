// Host-only weight layout code: file-format tensors -> the device layouts of
// kernels.h (lane-order linear weights, embedding-table planes, LN-fold constants).
// No HIP here: repack.cpp builds with a plain host compiler.
#pragma once

#include "host_common.h"

namespace emb {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One host-side staged buffer of the replica.
struct Piece {
    std::vector<uint8_t> bytes;
    size_t off = 0;
};

// Linear weight [N][K] (the parts' file rows, concatenated along N) -> lane order:
// qs, and for the quantized formats the d (and m) planes.  fmt_dev FMT_F32: the
// [hi | lo] f16 pairs of repack_linear_f32 (K_out = 2K).
void repack_linear(const std::vector<const HostTensor *> &parts, int fmt_dev, Piece &qs, Piece &dpl, Piece &mpl,
                   int &N_out, int &K_out);
void repack_linear_f32(const std::vector<const HostTensor *> &parts, Piece &qs, Piece &dpl, Piece &mpl, int &N_out,
                       int &K_out);
// LN fold constants c1 = W gamma, c2 = bias + W beta of a projection; exact: W as
// the f32 value (f32 files), else rounded once to f16 as the GEMM multiplies it.
void fold_ln(const std::vector<const HostTensor *> &parts, const std::vector<const HostTensor *> &bias,
             const HostTensor &gamma, const HostTensor &beta, Piece &c1, Piece &c2, bool exact);
// Embedding table in its file format -> aligned planes.
void repack_table(const HostTensor &t, Piece &qs, Piece &dpl, Piece &mpl);

}  // namespace emb
