// pzg_unlzw_kernel.h -- unlzw_kernel: LZW streams (TIFF Compression 5, PDF LZWDecode) decoded one wavefront a stream
// (pzg_unlzw_many; unlzw_core.h).  Like pzg_unshuffle_kernel.h it is compiled with pzg_api.cpp, its only includer: the code objects
// of pzg_kernels.hip and pzg_kernels_b.hip stay what they were.
// The workgroup is one wave; its LDS is the position array of the stream it decodes (Unlzw::Table, 15,360 bytes: ten workgroups
// to a CU by the 160 KiB of LDS).  The grid's x strides over the streams, a workgroup a stream up to UNLZW_GRID: streams are of any
// length, and the dispatcher hands the next one to whichever CU has room.
#pragma once
#include "unlzw_core.h"
#include "pzg_launch.h"

namespace pzg {

constexpr uint32_t UNLZW_GRID = 1u << 20;

__global__ __launch_bounds__(64) void unlzw_kernel(UnlzwArgs a)
{
    __shared__ Unlzw::Table table;
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const uint64_t in_len = uni64(a.in_len[i]), cap = uni64(a.out_cap[i]);
        const uint8_t *in = a.in_base + uni64(a.in_off[i]);
        uint8_t *out = a.out_base + uni64(a.out_off[i]);
        const Unlzw::Result r = Unlzw::stream(in, in_len, out, cap, a.early_change, table);
        if (threadIdx.x == 0) {
            a.status[i] = r.status;
            a.out_len[i] = r.out_len;
            if (a.detail) {
                a.detail[2 * i] = r.d0;
                a.detail[2 * i + 1] = r.d1;
            }
        }
        __syncthreads();
    }
}

inline hipError_t launch_unlzw(const UnlzwArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(unlzw_kernel, dim3(a.n < UNLZW_GRID ? a.n : UNLZW_GRID), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pzg
