// qgd_monitor_dev.hpp -- the skeleton of a run monitor, written once for the three blocks (qgd_monitor.hip: the flow block of a QGDFoam
// case; qgd_monitor_species.hip: its species block; qgd_qhd_monitor.hip: the block of a QHDFoam / SRFQHDFoam case).  A block is three
// launches: a cell kernel (one partial row per workgroup), a patch kernel (one partial row per chunk of <= 256 faces of one patch) and a
// fold kernel <<<1, 256>>> that folds both and writes the result block.  Here is everything in them that only initialises, compares,
// folds and stores; the per-cell and per-face arithmetic stays in the kernels.
//   the pairs        ArgVal {value, label}, argMin / argMax (ties to the lowest label), keepExtrema (a lane's update)
//   the fixed trees  waveFold / blockFold (lanes by shuffles in halving offsets, the four waves through LDS in wave order)
//   a lane's row     noExtrema, markNonFinite, keepFinite, storeCellRow: sums | EXTREMA x {min, label, max, label} | non-finite count,
//                    lowest label; storePatchRow
//   the row folds    foldColumn, foldExtremum, foldNonFinite, foldPatches: thread t takes rows r0 + t, r0 + t + 256, ... of [r0, r1) in
//                    ascending order, then the block tree -- fixed for a given grid and chunk table; the row length is a run-time value
//   the stores       storeExtremum (NaN, -1 where no cell had a finite value), NonFinite::first (-1: none), monitorHeader
// What the monitors promise follows from these alone: extrema over finite cells only, ties to the lowest label, -1 / NaN for "none",
// every sum in an order that depends on the mesh and the specification only.  (Ghost cells are kept out by the cell kernels' ranges.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "qgd_device.hpp"

namespace qgd {

#define QGD_MON_BLOCK 256
#define QGD_MON_NOLABEL 9007199254740992.0   // 2^53: above every label; "no finite value seen"

struct ArgVal { double v, l; };
// ties go to the lowest label
__device__ __forceinline__ ArgVal argMin(const ArgVal a, const ArgVal b) { return (b.v < a.v || (b.v == a.v && b.l < a.l)) ? b : a; }
__device__ __forceinline__ ArgVal argMax(const ArgVal a, const ArgVal b) { return (b.v > a.v || (b.v == a.v && b.l < a.l)) ? b : a; }
__device__ __forceinline__ ArgVal noMin() { return ArgVal{INFINITY, QGD_MON_NOLABEL}; }
__device__ __forceinline__ ArgVal noMax() { return ArgVal{-INFINITY, QGD_MON_NOLABEL}; }
// a lane meets its cells in ascending label order: the first one met stays on a tie
__device__ __forceinline__ void keepExtrema(ArgVal& lo, ArgVal& hi, const double v, const double label) {
    if (v < lo.v) lo = ArgVal{v, label};
    if (v > hi.v) hi = ArgVal{v, label};
}

struct OpSum { __device__ static double f(double a, double b) { return a + b; } };
struct OpMin { __device__ static double f(double a, double b) { return fmin(a, b); } };
struct OpMax { __device__ static double f(double a, double b) { return fmax(a, b); } };

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

// ---- what a lane of a cell kernel gathers, and the row its workgroup writes ---------------------------------------------------------------
// The accumulators themselves (s[], lo[] / hi[], bad, badLabel) are plain locals of the cell kernels, and the loop over a cell's values is
// theirs: gathered into one struct, or with that loop in here, monitorCellKernel comes out with other registers and measurably slower
// (one struct: + 0.5 % per sample; the loop in here: 138 VGPRs for 106, 3 waves per SIMD for 4).
template <int EXTREMA>
__device__ __forceinline__ void noExtrema(ArgVal (&lo)[EXTREMA], ArgVal (&hi)[EXTREMA]) {
#pragma unroll
    for (int k = 0; k < EXTREMA; ++k) { lo[k] = noMin(); hi[k] = noMax(); }
}
// a cell whose state is not finite: counted and named; the caller keeps it out of the extrema
__device__ __forceinline__ void markNonFinite(double& bad, double& badLabel, const double label) {
    bad += 1.0;
    badLabel = fmin(badLabel, label);
}
// one value of a cell whose state is finite; a value that is not finite all the same (a quotient, say) is skipped
__device__ __forceinline__ void keepFinite(ArgVal& lo, ArgVal& hi, const double v, const double label) {
    if (isFiniteD(v)) keepExtrema(lo, hi, v, label);
}
// row of SUMS + 4 EXTREMA + 2 doubles: sums | EXTREMA x {min, label, max, label} | non-finite count, lowest label.  sh: 8 doubles
template <int SUMS, int EXTREMA>
__device__ __forceinline__ void storeCellRow(const double (&s)[SUMS], const ArgVal (&lo)[EXTREMA], const ArgVal (&hi)[EXTREMA], const double bad,
                                             const double badLabel, double* row, double* sh) {
#pragma unroll
    for (int k = 0; k < SUMS; ++k) {
        const double r = blockFold<OpSum>(s[k], sh);
        if (threadIdx.x == 0) row[k] = r;
    }
#pragma unroll
    for (int k = 0; k < EXTREMA; ++k) {
        const ArgVal a = blockFoldArg<false>(lo[k], sh);
        const ArgVal b = blockFoldArg<true>(hi[k], sh);
        if (threadIdx.x == 0) {
            double* e = row + SUMS + 4 * k;
            e[0] = a.v; e[1] = a.l; e[2] = b.v; e[3] = b.l;
        }
    }
    const double nb = blockFold<OpSum>(bad, sh);
    const double lb = blockFold<OpMin>(badLabel, sh);
    if (threadIdx.x == 0) { row[SUMS + 4 * EXTREMA] = nb; row[SUMS + 4 * EXTREMA + 1] = lb; }
}

// the row of a chunk: every lane's N terms (zero past the chunk's end) summed over the workgroup.  sh: 4 doubles
template <int N>
__device__ __forceinline__ void storePatchRow(const double (&s)[N], double* row, double* sh) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double r = blockFold<OpSum>(s[k], sh);
        if (threadIdx.x == 0) row[k] = r;
    }
}

// ---- the folds of the fold kernels: rows [r0, r1) of rowLen doubles, results valid in thread 0 ----------------------------------------------
template <class Op>
__device__ __forceinline__ double foldColumn(const double* rows, const size_t rowLen, const int col, const int r0, const int r1, const double start,
                                             double* sh) {
    double x = start;
    for (int r = r0 + threadIdx.x; r < r1; r += QGD_MON_BLOCK) x = Op::f(x, rows[r * rowLen + col]);
    return blockFold<Op>(x, sh);
}
// the {min, label, max, label} at columns col .. col + 3.  sh: 8 doubles
struct MinMax { ArgVal lo, hi; };
__device__ __forceinline__ MinMax foldExtremum(const double* rows, const size_t rowLen, const int col, const int r0, const int r1, double* sh) {
    ArgVal a = noMin(), b = noMax();
    for (int r = r0 + threadIdx.x; r < r1; r += QGD_MON_BLOCK) {
        const double* e = rows + r * rowLen + col;
        a = argMin(a, ArgVal{e[0], e[1]});
        b = argMax(b, ArgVal{e[2], e[3]});
    }
    a = blockFoldArg<false>(a, sh);
    b = blockFoldArg<true>(b, sh);
    return MinMax{a, b};
}
// masked: the kernel's own reason for "none" (a quantity the state does not hold yet)
__device__ __forceinline__ void storeExtremum(double* ex, const MinMax e, const bool masked) {
    const double nan = __builtin_nan("");
    const bool none = e.lo.l >= QGD_MON_NOLABEL || masked;   // no cell with a finite value
    ex[0] = none ? nan : e.lo.v; ex[1] = none ? -1.0 : e.lo.l;
    ex[2] = none ? nan : e.hi.v; ex[3] = none ? -1.0 : e.hi.l;
}
// the {count, lowest label} at columns col, col + 1
struct NonFinite {
    double count, label;
    __device__ __forceinline__ double first() const { return label >= QGD_MON_NOLABEL ? -1.0 : label; }
};
__device__ __forceinline__ NonFinite foldNonFinite(const double* rows, const size_t rowLen, const int col, const int r0, const int r1, double* sh) {
    double nb = 0.0, lb = QGD_MON_NOLABEL;
    for (int r = r0 + threadIdx.x; r < r1; r += QGD_MON_BLOCK) {
        const double* e = rows + r * rowLen + col;
        nb += e[0];
        lb = fmin(lb, e[1]);
    }
    nb = blockFold<OpSum>(nb, sh);
    lb = blockFold<OpMin>(lb, sh);
    return NonFinite{nb, lb};
}
// header words 0..5 of the flow block and of the QHD block (6 and 7 are the kernel's own)
__device__ __forceinline__ void monitorHeader(double* hd, const MonitorView& mv, const int fluxState, const NonFinite nf) {
    hd[0] = (double)(mv.ownedEnd - mv.ownedBegin);
    hd[1] = (double)fluxState;
    hd[2] = (double)mv.nProbes;
    hd[3] = (double)mv.nPatches;
    hd[4] = nf.count;
    hd[5] = nf.first();
}
// the patch table: a patch's chunks are consecutive rows of `part`; isNan(k) is the kernel's mask of column k
template <class Mask>
__device__ __forceinline__ void foldPatches(const MonitorView& mv, const double* part, const int rowLen, double* pa, double* sh, const Mask isNan) {
    for (int p = 0; p < mv.nPatches; ++p) {
        const int r0 = mv.patchChunk[p], r1 = mv.patchChunk[p + 1];
        for (int k = 0; k < rowLen; ++k) {
            const double x = foldColumn<OpSum>(part, (size_t)rowLen, k, r0, r1, 0.0, sh);
            if (threadIdx.x == 0) pa[(size_t)p * rowLen + k] = isNan(k) ? __builtin_nan("") : x;
        }
    }
}

}  // namespace qgd
