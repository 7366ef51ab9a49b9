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
#include "qgd_monitor_dev.hpp"   // the row stores, the folds and the "none" rules every block shares

namespace qgd {

namespace {
constexpr MonitorShape SH = kFlowMonitorShape;
}

// ---- cells -------------------------------------------------------------------------------------------------------------------------
// row of SH.cellRow() doubles per workgroup: 8 sums | 5 x {min, label, max, label} | non-finite count, lowest label
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorCellKernel(const MonitorView mv, const MeshView m, const CaseView c, const GasModel g) {
    __shared__ double sh[8];
    double s[SH.sums];
#pragma unroll
    for (int k = 0; k < SH.sums; ++k) s[k] = 0.0;
    ArgVal lo[SH.extrema], hi[SH.extrema];
    noExtrema(lo, hi);
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
            markNonFinite(bad, badLabel, label);
            continue;   // extrema are taken over the cells whose state is finite
        }
        const double magU = sqrt(u2);
        const double val[SH.extrema] = {a.rho, a.p, a.e / g.Cv, magU, magU / cs};
#pragma unroll
        for (int k = 0; k < SH.extrema; ++k) keepFinite(lo[k], hi[k], val[k], label);
    }
    storeCellRow(s, lo, hi, bad, badLabel, mv.cellPart + (size_t)blockIdx.x * SH.cellRow(), sh);
}

// ---- patch faces -------------------------------------------------------------------------------------------------------------------
// one workgroup per chunk (<= 256 consecutive entries of the face list, all of one patch); row of SH.patchRow doubles:
// |Sf|, the five net fluxes, p_b Sf
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorPatchKernel(const MonitorView mv, const MeshView m, const CaseView c) {
    __shared__ double sh[4];
    const int first = mv.chunkStart[blockIdx.x], n = mv.chunkStart[blockIdx.x + 1] - first;
    double s[SH.patchRow];
#pragma unroll
    for (int k = 0; k < SH.patchRow; ++k) s[k] = 0.0;
    if ((int)threadIdx.x < n) {
        const int b = mv.faceList[first + threadIdx.x];   // boundary face index
        const size_t f = (size_t)m.nIF + b;
        s[0] = m.magSf[f];
#pragma unroll
        for (int k = 0; k < 5; ++k) s[1 + k] = c.flux[(size_t)k * m.nF + f];
        const double pb = c.bA[b].p;
        s[6] = pb * m.Sx[f]; s[7] = pb * m.Sy[f]; s[8] = pb * m.Sz[f];
    }
    storePatchRow(s, mv.patchPart + (size_t)blockIdx.x * SH.patchRow, sh);
}

// ---- fold --------------------------------------------------------------------------------------------------------------------------
// header: owned cells, fluxState, probes, patches, non-finite cells, the first of them | deltaT, the one before
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorFoldKernel(const MonitorView mv, const CaseView c, const GasModel g, const int nCellRows,
                                                                  const int fluxState, double* __restrict__ out) {
    __shared__ double sh[8];
    const int t = threadIdx.x;
    double* hd = out + mv.off[0];
    double* in = out + mv.off[1];
    for (int k = 0; k < SH.sums; ++k) {
        const double x = foldColumn<OpSum>(mv.cellPart, SH.cellRow(), k, 0, nCellRows, 0.0, sh);
        if (t == 0) in[k] = x;
    }
    double* ex = out + mv.off[2];
    for (int k = 0; k < SH.extrema; ++k) {
        const MinMax e = foldExtremum(mv.cellPart, SH.cellRow(), SH.sums + 4 * k, 0, nCellRows, sh);
        if (t == 0) storeExtremum(ex + 4 * k, e, false);
    }
    const NonFinite nf = foldNonFinite(mv.cellPart, SH.cellRow(), SH.sums + 4 * SH.extrema, 0, nCellRows, sh);
    if (t == 0) {
        monitorHeader(hd, mv, fluxState, nf);
        hd[6] = c.dt[0];
        hd[7] = c.dt[1];
    }
    // probes: rho, Ux, Uy, Uz, p, T, e
    double* pr = out + mv.off[3];
    for (int i = t; i < mv.nProbes; i += QGD_MON_BLOCK) {
        const int cell = mv.probeCell[i];
        double* o = pr + (size_t)i * SH.probeRow;
        if (cell < 0) {
#pragma unroll
            for (int k = 0; k < SH.probeRow; ++k) o[k] = __builtin_nan("");
        } else {
            const RecA a = c.A[cell];
            o[0] = a.rho; o[1] = a.ux; o[2] = a.uy; o[3] = a.uz; o[4] = a.p; o[5] = a.e / g.Cv; o[6] = a.e;
        }
    }
    // patches.  The flux columns 1..5 -- fluxState 0: nothing assembled yet; 2: implicitDiffusion, where flux[1..4] hold the explicit part only
    foldPatches(mv, mv.patchPart, SH.patchRow, out + mv.off[4], sh,
                [=](int k) { return k >= 1 && k <= 5 && (fluxState == 0 || (fluxState == 2 && k >= 2)); });
}

void launchMonitorSample(hipStream_t s, const MonitorView& mv, const MeshView& m, const CaseView& c, const GasModel& g, int fluxState, double* out) {
    const int64_t nOwned = (int64_t)mv.ownedEnd - mv.ownedBegin;
    const int grid = (int)std::min<int64_t>((nOwned + QGD_MON_BLOCK - 1) / QGD_MON_BLOCK, QGD_MONITOR_BLOCKS);
    if (grid > 0) monitorCellKernel<<<grid, QGD_MON_BLOCK, 0, s>>>(mv, m, c, g);
    if (mv.nChunks > 0) monitorPatchKernel<<<mv.nChunks, QGD_MON_BLOCK, 0, s>>>(mv, m, c);
    monitorFoldKernel<<<1, QGD_MON_BLOCK, 0, s>>>(mv, c, g, grid, fluxState, out);
}

}  // namespace qgd
