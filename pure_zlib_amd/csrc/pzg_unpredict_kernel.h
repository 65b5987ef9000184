// pzg_unpredict_kernel.h -- unpredict_kernel: TIFF Predictor 2 undone and strips / tiles clipped to their windows, the rows of every
// job over the grid's y (pzg_unpredict_many; unpredict_core.h).  Like pzg_expand_kernel.h it is compiled with pzg_api.cpp, its only
// includer: the code objects of pzg_kernels.hip and pzg_kernels_b.hip stay what they were.
// The grid is that of expand_kernel: x strides over the jobs, y is the slice -- the wave of slice s takes the row groups s, s + slices,
// ... of each of its jobs -- so every (job, slice) pair is visited exactly once.  The workgroup is one wave and has no LDS.
// The slices are chosen by the launch's size alone (the descriptors are device memory, the host does not read them): few jobs get
// many slices -- one strip can be a whole image -- and thousands of tiles get four, about 32 Ki waves either way.  A wave whose
// slice has no rows of a job leaves it after reading its descriptor.
#pragma once
#include "unpredict_core.h"
#include "pzg_launch.h"

namespace pzg {

constexpr uint32_t UNPREDICT_GRID = 1u << 20, UNPREDICT_WAVES = 32768u, UNPREDICT_MIN_SLICES = 4u, UNPREDICT_MAX_SLICES = 4096u;

inline uint32_t unpredict_slices(uint32_t n)
{
    const uint32_t s = (UNPREDICT_WAVES + n - 1u) / n;
    return s < UNPREDICT_MIN_SLICES ? UNPREDICT_MIN_SLICES : s > UNPREDICT_MAX_SLICES ? UNPREDICT_MAX_SLICES : s;
}

__global__ __launch_bounds__(64) void unpredict_kernel(UnpredictArgs a)
{
    const Unpredict::Desc *desc = (const Unpredict::Desc *)a.desc;
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const Unpredict::Desc D = Unpredict::fetch(desc + i);
        Unpredict::job(a.src_base, uni64(a.src_len[i]), a.dst_base, D, blockIdx.y, gridDim.y, a.status + i, a.detail ? a.detail + 2 * (size_t)i : nullptr);
    }
}

inline hipError_t launch_unpredict(const UnpredictArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(unpredict_kernel, dim3(a.n < UNPREDICT_GRID ? a.n : UNPREDICT_GRID, unpredict_slices(a.n)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pzg
