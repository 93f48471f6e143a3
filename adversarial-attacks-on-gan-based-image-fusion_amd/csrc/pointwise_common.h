// What the two pointwise translation units (pointwise.hip, attack_step.hip) share: the block size,
// the grid size of a grid-stride loop and the launch-and-return of their entry points.
#pragma once
#include "mia_common.h"

namespace mia {

constexpr int TPB = 256;

static inline int blocks_for(int64_t n, int per_block = TPB, int cap = 1 << 20) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  return (int)(b > cap ? cap : b);
}

}  // namespace mia

#define MIA_LAUNCH(kern, grid, block, shmem, ...)                                  \
  do {                                                                             \
    hipLaunchKernelGGL(kern, grid, block, shmem, (hipStream_t)stream, __VA_ARGS__); \
    return check_launch(#kern);                                                    \
  } while (0)
