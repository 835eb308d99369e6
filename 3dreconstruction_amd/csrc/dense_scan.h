// The ordered compaction of fuse.hip and mesh.hip: a lane's place in the output
// is its workgroup's base (the exclusive int64 prefix of the workgroups' counts)
// + its rank inside the workgroup.  No atomics: the order is the schedule's no
// more.  A workgroup is 256 lanes, four wavefronts; wave_lds is four LDS words;
// every lane must reach a call (they hold __syncthreads()).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfm {

constexpr int kDenseBlock = 256;

// the sum of v over the workgroup's lanes before this one; *total: over all of
// them.  wave_lds may be used again right after the call.
__device__ inline int32_t block_exclusive(int32_t v, int32_t* wave_lds, int32_t* total) {
    int32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(incl, o);
        if ((int)(threadIdx.x & 63) >= o) incl += up;
    }
    if ((threadIdx.x & 63) == 63) wave_lds[threadIdx.x >> 6] = incl;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < (int)(threadIdx.x >> 6)) before += wave_lds[w];
        all += wave_lds[w];
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// The same for a flag, from the wavefronts' 64-bit ballots.  One barrier, none
// after the reads: a second call takes another wave_lds.
__device__ inline int32_t block_ballot_rank(bool pred, int32_t* wave_lds, int32_t* total) {
    const unsigned long long set = __ballot(pred);
    if ((threadIdx.x & 63) == 0) wave_lds[threadIdx.x >> 6] = (int32_t)__popcll(set);
    __syncthreads();
    *total = (wave_lds[0] + wave_lds[1]) + (wave_lds[2] + wave_lds[3]);
    int32_t before = (int32_t)__popcll(set & ((1ull << (threadIdx.x & 63)) - 1ull));
    for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) before += wave_lds[w];
    return before;
}

// Array blockIdx.x of count [gridDim.x][n] and base [gridDim.x][n + 1]: base[k] =
// count[0] + .. + count[k - 1], base[n] = the total; 256 counts a step.
static __global__ __launch_bounds__(kDenseBlock) void dense_scan_kernel(const int32_t* count, int64_t n, int64_t* base) {
    __shared__ int32_t wave_lds[4];
    count += (int64_t)blockIdx.x * n;
    base += (int64_t)blockIdx.x * (n + 1);
    int64_t carry = 0;   // the same in every lane
    for (int64_t k0 = 0; k0 < n; k0 += kDenseBlock) {
        const int64_t k = k0 + threadIdx.x;
        int32_t all;
        const int32_t before = block_exclusive(k < n ? count[k] : 0, wave_lds, &all);
        if (k < n) base[k] = carry + (int64_t)before;
        carry += all;
    }
    if (threadIdx.x == 0) base[n] = carry;
}

}  // namespace sfm
