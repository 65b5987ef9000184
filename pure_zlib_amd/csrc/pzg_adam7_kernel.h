// pzg_adam7_kernel.h -- adam7_kernel: Adam7 deinterlacing, the rows of every image over Adam7::SLICES waves (pzg_adam7_many;
// adam7_core.h).  Like pzg_unfilter_kernel.h it is compiled with pzg_api.cpp, its only includer: the code objects of
// pzg_kernels.hip and pzg_kernels_b.hip stay what they were.
// The grid is two-dimensional because the host does not read device arrays and so cannot size it by the heights: x strides over
// the images, y is the slice -- the wave of slice s takes the rows s, s + SLICES, ... of each of its images.
#pragma once
#include "adam7_core.h"
#include "pzg_launch.h"

namespace pzg {

constexpr uint32_t ADAM7_GRID = 1u << 20;

__global__ __launch_bounds__(64) void adam7_kernel(Adam7Args a)
{
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        int32_t status;
        uint32_t d0, d1;
        Adam7::image(a.src_base + uni64(a.src_off[i]), a.dst_base + uni64(a.dst_off[i]), uni64(a.dst_stride[i]), uni(a.width[i]), uni(a.height[i]),
                     uni(a.pixel_bits[i]), blockIdx.y, gridDim.y, &status, &d0, &d1);
        if (threadIdx.x == 0 && blockIdx.y == 0) {
            a.status[i] = status;
            if (a.detail) {
                a.detail[2 * (size_t)i] = d0;
                a.detail[2 * (size_t)i + 1] = d1;
            }
        }
    }
}

inline hipError_t launch_adam7(const Adam7Args &a, hipStream_t stream)
{
    hipLaunchKernelGGL(adam7_kernel, dim3(a.n < ADAM7_GRID ? a.n : ADAM7_GRID, Adam7::SLICES), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pzg
