// The tiling and chunking constants of the passes over a whole data set: moments.hip (weighted moments of the cross-kernel) and
// sites.hip (Gaussian sites of a non-Gaussian likelihood), which builds its K blocks exactly as moments.hip does.
#pragma once
#include "common.h"

namespace vargp {

constexpr int kMoT = 64;               // tile side of Phi = columns of X per step
constexpr int kSiMaxMt = 4 * kMoT;     // sites.hip holds the K block of ALL Mt rows x kMoT columns in LDS: Mt above this has no fused pass
constexpr int kMoLD = kMoT + 1;
constexpr int kMoBK = 32;              // values of d per slab (D > kRbfDirectD)
constexpr int kMoDl = kRbfDirectD | 1; // row stride of the staged points (direct form)
constexpr int kMoTargetWg = 1024;
constexpr int kMoMinChunk = 256;
constexpr int kMoMaxChunks = 1024;

}  // namespace vargp
