// qgd_monitor_dev.hpp -- what the monitor passes share (qgd_monitor.hip: the flow block; qgd_monitor_species.hip: the species block): the
// {value, label} pairs of the extrema and the wave and workgroup folds.  Every fold is a fixed tree: lanes by shuffles in halving
// offsets, the four waves of a workgroup through LDS in wave order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace qgd {

#define QGD_MON_BLOCK 256
#define QGD_MON_NOLABEL 9007199254740992.0   // 2^53: above every label; "no finite value seen"

struct ArgVal { double v, l; };
// ties go to the lowest label
__device__ __forceinline__ ArgVal argMin(const ArgVal a, const ArgVal b) { return (b.v < a.v || (b.v == a.v && b.l < a.l)) ? b : a; }
__device__ __forceinline__ ArgVal argMax(const ArgVal a, const ArgVal b) { return (b.v > a.v || (b.v == a.v && b.l < a.l)) ? b : a; }

struct OpSum { __device__ static double f(double a, double b) { return a + b; } };
struct OpMin { __device__ static double f(double a, double b) { return fmin(a, b); } };

template <class Op>
__device__ __forceinline__ double waveFold(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = Op::f(x, __shfl_down(x, off, 64));
    return x;
}
template <bool MAX>
__device__ __forceinline__ ArgVal waveFoldArg(ArgVal x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ArgVal y;
        y.v = __shfl_down(x.v, off, 64);
        y.l = __shfl_down(x.l, off, 64);
        x = MAX ? argMax(x, y) : argMin(x, y);
    }
    return x;
}
// the four waves of a workgroup through LDS, in wave order; the result is valid in thread 0.  sh: 4 doubles (8 for the pairs)
template <class Op>
__device__ __forceinline__ double blockFold(double x, double* sh) {
    x = waveFold<Op>(x);
    __syncthreads();   // sh may still be read from the fold before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return Op::f(Op::f(sh[0], sh[1]), Op::f(sh[2], sh[3]));
}
template <bool MAX>
__device__ __forceinline__ ArgVal blockFoldArg(ArgVal x, double* sh) {
    x = waveFoldArg<MAX>(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh[2 * (threadIdx.x >> 6)] = x.v; sh[2 * (threadIdx.x >> 6) + 1] = x.l; }
    __syncthreads();
    ArgVal r{sh[0], sh[1]};
#pragma unroll
    for (int w = 1; w < 4; ++w) { const ArgVal y{sh[2 * w], sh[2 * w + 1]}; r = MAX ? argMax(r, y) : argMin(r, y); }
    return r;
}

__device__ __forceinline__ bool isFiniteD(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN and +-inf

}  // namespace qgd
