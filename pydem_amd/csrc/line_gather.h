// line_gather.h -- k_line_gather<T>: a column of a plane into a contiguous line.  tile.hip (pydem_tile_get_lines, the column get)
// and seam_get_lines of stage_kit.h launch it; internal linkage: a kernel of every unit that does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// `src[0], src[stride], ...` into dst[0 .. count - 1]
template <typename T>
__global__ void k_line_gather(const T *__restrict__ src, int64_t stride, int64_t count, T *__restrict__ dst)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) dst[k] = src[k * stride];
}

}  // namespace
