// pzg_expand_kernel.h -- expand_kernel: pixel expansion to RGBA8 / RGB8, the rows of every image over Expand::SLICES waves
// (pzg_expand_many; expand_core.h).  Like pzg_adam7_kernel.h it is compiled with pzg_api.cpp, its only includer: the code objects of
// pzg_kernels.hip and pzg_kernels_b.hip stay what they were.
// The grid is that of adam7_kernel: x strides over the images, y is the slice -- the wave of slice s takes the rows s, s + SLICES, ...
// of each of its images -- so every (image, slice) pair is visited exactly once and gridDim.y waves arrive at a palette image's counter.
// The workgroup is one wave; its 1 KiB of LDS holds the palette of the image it is at.
#pragma once
#include "expand_core.h"
#include "pzg_launch.h"

namespace pzg {

constexpr uint32_t EXPAND_GRID = 1u << 20;

__global__ __launch_bounds__(64) void expand_kernel(ExpandArgs a)
{
    __shared__ uint32_t pal[256];
    const Expand::Desc *desc = (const Expand::Desc *)a.desc;
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const Expand::Desc D = Expand::fetch(desc + i);
        Expand::image(a.src_base, a.dst_base, a.palette_base, D, pal, blockIdx.y, gridDim.y, a.scratch + 2 * (size_t)i, a.status + i,
                      a.detail ? a.detail + 2 * (size_t)i : nullptr);
    }
}

// (a.scratch has been zeroed on the same stream, in front of the launch)
inline hipError_t launch_expand(const ExpandArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(expand_kernel, dim3(a.n < EXPAND_GRID ? a.n : EXPAND_GRID, Expand::SLICES), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pzg
