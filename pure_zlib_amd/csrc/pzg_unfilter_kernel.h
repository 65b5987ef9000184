// pzg_unfilter_kernel.h -- unfilter_kernel: scanline unfiltering, a wave per image (pzg_unfilter_many; unfilter_core.h).  It has
// nothing of the inflate core in it and is compiled with pzg_api.cpp, its only includer: the code objects of pzg_kernels.hip and
// pzg_kernels_b.hip stay what they were, and every script that builds the library from its three translation units builds this too.
#pragma once
#include "pzg_launch.h"
#include "unfilter_core.h"

namespace pzg {

constexpr uint32_t UNFILTER_GRID = 1u << 20;

__global__ __launch_bounds__(64) void unfilter_kernel(UnfilterArgs a)
{
    for (uint32_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        int32_t status;
        uint32_t d0, d1;
        Unfilter::image(a.src_base + uni64(a.src_off[i]), uni64(a.src_len[i]), a.dst_base + uni64(a.dst_off[i]), uni64(a.dst_stride[i]),
                        uni(a.row_bytes[i]), uni(a.height[i]), uni(a.bpp[i]), &status, &d0, &d1);
        if (threadIdx.x == 0) {
            a.status[i] = status;
            if (a.detail) {
                a.detail[2 * (size_t)i] = d0;
                a.detail[2 * (size_t)i + 1] = d1;
            }
        }
    }
}

inline hipError_t launch_unfilter(const UnfilterArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(unfilter_kernel, dim3(a.n < UNFILTER_GRID ? a.n : UNFILTER_GRID), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pzg
