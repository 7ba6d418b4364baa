// corrmfma.hpp -- the matrix-core altcorr's own constants and parameters
// (corrmfma.hip: one wave per edge, windows read through the vector-memory
// path).  The window geometry, the box rule, the bilinear weights and
// cm_bilinear are corr.hpp's.
#pragma once

#include "corr.hpp"

namespace dpvo {

namespace cm {
constexpr int WAVES = 4;
constexpr int RS = 148;           // LDS row per patch pixel: the box's <= 144 pixels (+ pad: rows 4 apart, 16 banks apart)
constexpr int RL = corr::NP * RS; // per level
constexpr unsigned OOB = 0x80000000u;   // a buffer offset past every descriptor's range: the load returns 0
static_assert(corr::BOX * corr::BOX <= RS, "a raw row holds the whole box");
}  // namespace cm

struct CorrMfmaParams {
    const half_t* gt;   // [N1][9][128] transposed patch features
    int N1;
    const float* coords;
    int64_t c_s[5];
    const int64_t* ii;
    const int64_t* jj;
    int E;
    const half_t* fmap[2];
    int64_t f_s1[2];
    int N2[2], H2[2], W2[2];
    int64_t rowb[2];          // row stride in bytes
    int pixb[2];              // pixel stride in bytes
    int rowext[2];            // bytes from a row's first pixel to the end of its last
    int frameext[2];          // bytes from a frame's first pixel to the end of its last
    float scale[2];
    half_t* out;
    int64_t o_e;
    const int* order;   // optional edge visiting order (edges grouped by target frame), NULL = 0..E-1
};

}  // namespace dpvo
