// The nearest-neighbour search of chamfer.hip as a host-side launch, for the other translation units that need the SAME kernel
// (points_fit.hip: the one-way observation -> vertex search of the points3d term).
#pragma once
#include "common.h"

namespace ha {

// For every point of xyz1 [b,n,3]: squared distance to, and int32 index of, the nearest point of xyz2 [b,m,3] (chamfer_nn_kernel:
// (dx*dx + dy*dy) + dz*dz without contraction, lowest index on ties).  b <= 65535; checks the launch like every entry point.
int chamfer_nn_launch(int b, int n, const float* xyz1, int m, const float* xyz2, float* dist, int32_t* idx, hipStream_t st);

}  // namespace ha
