// pzg_unshuffle_kernel.h -- unshuffle_kernel: the byte-plane transpose undone, with TIFF Predictor 3's byte-wise sum in front of it or
// without, and strips / tiles clipped to their windows, the rows of every job over the grid's y (pzg_unshuffle_many; unshuffle_core.h).
// Like pzg_unpredict_kernel.h it is compiled with pzg_api.cpp, its only includer: the code objects of pzg_kernels.hip and
// pzg_kernels_b.hip stay what they were.
// The grid is that of the Predictor 2 stage: x strides over the jobs, y is the slice -- the wave of slice s takes the row groups s,
// s + slices, ... of each of its jobs -- so every (job, slice) pair is visited exactly once.  The workgroup is one wave and has no LDS.
// The slices are chosen by the launch's size alone (the descriptors are device memory, the host does not read them): few jobs get
// many slices -- one strip can be a whole image -- and thousands of tiles get four, about 32 Ki waves either way.
#pragma once
#include "unshuffle_core.h"
#include "pzg_launch.h"

namespace pzg {

constexpr uint32_t UNSHUFFLE_GRID = 1u << 20, UNSHUFFLE_WAVES = 32768u, UNSHUFFLE_MIN_SLICES = 4u, UNSHUFFLE_MAX_SLICES = 4096u;

inline uint32_t unshuffle_slices(uint32_t n)
{
    const uint32_t s = (UNSHUFFLE_WAVES + n - 1u) / n;
    return s < UNSHUFFLE_MIN_SLICES ? UNSHUFFLE_MIN_SLICES : s > UNSHUFFLE_MAX_SLICES ? UNSHUFFLE_MAX_SLICES : s;
}

__global__ __launch_bounds__(64) void unshuffle_kernel(UnshuffleArgs a)
{
    const Unshuffle::Desc *desc = (const Unshuffle::Desc *)a.desc;
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const Unshuffle::Desc D = Unshuffle::fetch(desc + i);
        Unshuffle::job(a.src_base, uni64(a.src_len[i]), a.dst_base, D, blockIdx.y, gridDim.y, a.status + i, a.detail ? a.detail + 2 * (size_t)i : nullptr);
    }
}

inline hipError_t launch_unshuffle(const UnshuffleArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(unshuffle_kernel, dim3(a.n < UNSHUFFLE_GRID ? a.n : UNSHUFFLE_GRID, unshuffle_slices(a.n)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pzg
