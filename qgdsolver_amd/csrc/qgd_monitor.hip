// qgd_monitor.hip -- run monitors of a resident QGDFoam case (gfx950, wave64): volume integrals, extrema with their cells, the first
// non-finite cell, probes and patch totals of the net face fluxes, formed on the device from the records and CaseView::flux.
//
// Three launches per sample: monitorCellKernel (one partial row per workgroup), monitorPatchKernel (one partial row per chunk of a
// patch's face list), monitorFoldKernel<<<1, 256>>> (folds both, gathers the probes, writes the result block).  No float atomics, no
// in-launch ticket: the order of every sum depends on the mesh and the specification only (lane l of workgroup b takes cells
// b * 256 + l, + grid * 256, ... in ascending label order; lanes, waves, workgroups and chunks are folded in fixed trees), so two
// samples of one state are bitwise equal whichever step path produced it.  Nothing here writes to the case.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "qgd_device.hpp"
#include "qgd_monitor_dev.hpp"   // the folds and the {value, label} pairs, shared with the species block

namespace qgd {

// ---- cells -------------------------------------------------------------------------------------------------------------------------
// row of QGD_MONITOR_CELL_ROW doubles per workgroup: 8 sums | 5 x {min, label, max, label} | non-finite count, lowest label
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorCellKernel(const MonitorView mv, const MeshView m, const CaseView c, const GasModel g) {
    __shared__ double sh[8];
    double s[QGD_MONITOR_SUMS];
#pragma unroll
    for (int k = 0; k < QGD_MONITOR_SUMS; ++k) s[k] = 0.0;
    ArgVal lo[QGD_MONITOR_EXTREMA], hi[QGD_MONITOR_EXTREMA];
#pragma unroll
    for (int k = 0; k < QGD_MONITOR_EXTREMA; ++k) { lo[k] = ArgVal{INFINITY, QGD_MON_NOLABEL}; hi[k] = ArgVal{-INFINITY, QGD_MON_NOLABEL}; }
    double bad = 0.0, badLabel = QGD_MON_NOLABEL;
    const int64_t stride = (int64_t)gridDim.x * QGD_MON_BLOCK;
    for (int64_t i = (int64_t)mv.ownedBegin + (int64_t)blockIdx.x * QGD_MON_BLOCK + threadIdx.x; i < mv.ownedEnd; i += stride) {
        const RecA a = c.A[i];
        const double cs = c.B[i].c, V = m.V[i];
        const double label = mv.cellGlobal ? (double)mv.cellGlobal[i] : (double)(i + mv.cellGlobalOffset);
        const double u2 = a.ux * a.ux + a.uy * a.uy + a.uz * a.uz;
        const double ke = 0.5 * u2;
        const double rE = c.rE ? c.rE[i] : a.rho * (a.e + ke);
        s[0] += V;
        s[1] += a.rho * V;
        s[2] += a.rho * a.ux * V;
        s[3] += a.rho * a.uy * V;
        s[4] += a.rho * a.uz * V;
        s[5] += rE * V;
        s[6] += a.rho * a.e * V;
        s[7] += a.rho * ke * V;
        if (!(isFiniteD(a.rho) && isFiniteD(a.p) && isFiniteD(a.e) && isFiniteD(a.ux) && isFiniteD(a.uy) && isFiniteD(a.uz))) {
            bad += 1.0;
            badLabel = fmin(badLabel, label);
            continue;   // extrema are taken over the cells whose state is finite
        }
        const double magU = sqrt(u2);
        const double val[QGD_MONITOR_EXTREMA] = {a.rho, a.p, a.e / g.Cv, magU, magU / cs};
#pragma unroll
        for (int k = 0; k < QGD_MONITOR_EXTREMA; ++k) {
            if (!isFiniteD(val[k])) continue;
            if (val[k] < lo[k].v) lo[k] = ArgVal{val[k], label};   // ascending labels per lane: the first one met stays on a tie
            if (val[k] > hi[k].v) hi[k] = ArgVal{val[k], label};
        }
    }
    double* row = mv.cellPart + (size_t)blockIdx.x * QGD_MONITOR_CELL_ROW;
#pragma unroll
    for (int k = 0; k < QGD_MONITOR_SUMS; ++k) {
        const double r = blockFold<OpSum>(s[k], sh);
        if (threadIdx.x == 0) row[k] = r;
    }
#pragma unroll
    for (int k = 0; k < QGD_MONITOR_EXTREMA; ++k) {
        const ArgVal a = blockFoldArg<false>(lo[k], sh);
        const ArgVal b = blockFoldArg<true>(hi[k], sh);
        if (threadIdx.x == 0) {
            double* e = row + QGD_MONITOR_SUMS + 4 * k;
            e[0] = a.v; e[1] = a.l; e[2] = b.v; e[3] = b.l;
        }
    }
    const double nb = blockFold<OpSum>(bad, sh);
    const double lb = blockFold<OpMin>(badLabel, sh);
    if (threadIdx.x == 0) { row[QGD_MONITOR_SUMS + 4 * QGD_MONITOR_EXTREMA] = nb; row[QGD_MONITOR_SUMS + 4 * QGD_MONITOR_EXTREMA + 1] = lb; }
}

// ---- patch faces -------------------------------------------------------------------------------------------------------------------
// one workgroup per chunk (<= 256 consecutive entries of the face list, all of one patch); row of QGD_MONITOR_PATCH_ROW doubles:
// |Sf|, the five net fluxes, p_b Sf
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorPatchKernel(const MonitorView mv, const MeshView m, const CaseView c) {
    __shared__ double sh[4];
    const int first = mv.chunkStart[blockIdx.x], n = mv.chunkStart[blockIdx.x + 1] - first;
    double s[QGD_MONITOR_PATCH_ROW];
#pragma unroll
    for (int k = 0; k < QGD_MONITOR_PATCH_ROW; ++k) s[k] = 0.0;
    if ((int)threadIdx.x < n) {
        const int b = mv.faceList[first + threadIdx.x];   // boundary face index
        const size_t f = (size_t)m.nIF + b;
        s[0] = m.magSf[f];
#pragma unroll
        for (int k = 0; k < 5; ++k) s[1 + k] = c.flux[(size_t)k * m.nF + f];
        const double pb = c.bA[b].p;
        s[6] = pb * m.Sx[f]; s[7] = pb * m.Sy[f]; s[8] = pb * m.Sz[f];
    }
    double* row = mv.patchPart + (size_t)blockIdx.x * QGD_MONITOR_PATCH_ROW;
#pragma unroll
    for (int k = 0; k < QGD_MONITOR_PATCH_ROW; ++k) {
        const double r = blockFold<OpSum>(s[k], sh);
        if (threadIdx.x == 0) row[k] = r;
    }
}

// ---- fold --------------------------------------------------------------------------------------------------------------------------
// thread t takes rows t, t + 256, ... in ascending order, then the block tree: fixed for a given grid and chunk table
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorFoldKernel(const MonitorView mv, const CaseView c, const GasModel g, const int nCellRows,
                                                                  const int fluxState, double* __restrict__ out) {
    __shared__ double sh[8];
    const int t = threadIdx.x;
    const double nan = __builtin_nan("");
    // header
    double* hd = out + mv.off[0];
    double* in = out + mv.off[1];
    for (int k = 0; k < QGD_MONITOR_SUMS; ++k) {
        double x = 0.0;
        for (int r = t; r < nCellRows; r += QGD_MON_BLOCK) x += mv.cellPart[(size_t)r * QGD_MONITOR_CELL_ROW + k];
        x = blockFold<OpSum>(x, sh);
        if (t == 0) in[k] = x;
    }
    double* ex = out + mv.off[2];
    for (int k = 0; k < QGD_MONITOR_EXTREMA; ++k) {
        ArgVal a{INFINITY, QGD_MON_NOLABEL}, b{-INFINITY, QGD_MON_NOLABEL};
        for (int r = t; r < nCellRows; r += QGD_MON_BLOCK) {
            const double* e = mv.cellPart + (size_t)r * QGD_MONITOR_CELL_ROW + QGD_MONITOR_SUMS + 4 * k;
            a = argMin(a, ArgVal{e[0], e[1]});
            b = argMax(b, ArgVal{e[2], e[3]});
        }
        a = blockFoldArg<false>(a, sh);
        b = blockFoldArg<true>(b, sh);
        if (t == 0) {
            const bool none = a.l >= QGD_MON_NOLABEL;   // no cell with a finite value
            ex[4 * k] = none ? nan : a.v; ex[4 * k + 1] = none ? -1.0 : a.l;
            ex[4 * k + 2] = none ? nan : b.v; ex[4 * k + 3] = none ? -1.0 : b.l;
        }
    }
    {
        double nb = 0.0, lb = QGD_MON_NOLABEL;
        for (int r = t; r < nCellRows; r += QGD_MON_BLOCK) {
            const double* e = mv.cellPart + (size_t)r * QGD_MONITOR_CELL_ROW + QGD_MONITOR_SUMS + 4 * QGD_MONITOR_EXTREMA;
            nb += e[0];
            lb = fmin(lb, e[1]);
        }
        nb = blockFold<OpSum>(nb, sh);
        lb = blockFold<OpMin>(lb, sh);
        if (t == 0) {
            hd[0] = (double)(mv.ownedEnd - mv.ownedBegin);
            hd[1] = (double)fluxState;
            hd[2] = (double)mv.nProbes;
            hd[3] = (double)mv.nPatches;
            hd[4] = nb;
            hd[5] = lb >= QGD_MON_NOLABEL ? -1.0 : lb;
            hd[6] = c.dt[0];
            hd[7] = c.dt[1];
        }
    }
    // probes: rho, Ux, Uy, Uz, p, T, e
    double* pr = out + mv.off[3];
    for (int i = t; i < mv.nProbes; i += QGD_MON_BLOCK) {
        const int cell = mv.probeCell[i];
        double* o = pr + (size_t)i * QGD_MONITOR_PROBE_ROW;
        if (cell < 0) {
#pragma unroll
            for (int k = 0; k < QGD_MONITOR_PROBE_ROW; ++k) o[k] = nan;
        } else {
            const RecA a = c.A[cell];
            o[0] = a.rho; o[1] = a.ux; o[2] = a.uy; o[3] = a.uz; o[4] = a.p; o[5] = a.e / g.Cv; o[6] = a.e;
        }
    }
    // patches: their chunks are consecutive rows
    double* pa = out + mv.off[4];
    for (int p = 0; p < mv.nPatches; ++p) {
        const int r0 = mv.patchChunk[p], r1 = mv.patchChunk[p + 1];
        for (int k = 0; k < QGD_MONITOR_PATCH_ROW; ++k) {
            double x = 0.0;
            for (int r = r0 + t; r < r1; r += QGD_MON_BLOCK) x += mv.patchPart[(size_t)r * QGD_MONITOR_PATCH_ROW + k];
            x = blockFold<OpSum>(x, sh);
            // fluxState 0: nothing assembled yet; 2: implicitDiffusion, where flux[1..4] hold the explicit part only
            const bool isFlux = k >= 1 && k <= 5;
            if (isFlux && (fluxState == 0 || (fluxState == 2 && k >= 2))) x = nan;
            if (t == 0) pa[(size_t)p * QGD_MONITOR_PATCH_ROW + k] = x;
        }
    }
}

void launchMonitorSample(hipStream_t s, const MonitorView& mv, const MeshView& m, const CaseView& c, const GasModel& g, int fluxState, double* out) {
    const int64_t nOwned = (int64_t)mv.ownedEnd - mv.ownedBegin;
    const int grid = (int)std::min<int64_t>((nOwned + QGD_MON_BLOCK - 1) / QGD_MON_BLOCK, QGD_MONITOR_BLOCKS);
    if (grid > 0) monitorCellKernel<<<grid, QGD_MON_BLOCK, 0, s>>>(mv, m, c, g);
    if (mv.nChunks > 0) monitorPatchKernel<<<mv.nChunks, QGD_MON_BLOCK, 0, s>>>(mv, m, c);
    monitorFoldKernel<<<1, QGD_MON_BLOCK, 0, s>>>(mv, c, g, grid, fluxState, out);
}

}  // namespace qgd
