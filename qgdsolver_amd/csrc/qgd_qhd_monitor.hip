// qgd_qhd_monitor.hip -- run monitor of a resident QHDFoam / SRFQHDFoam case (gfx950, wave64): volume integrals, the body force the next
// step's cell update forms from the state, the continuity error of the pressure solve (the signed sum of phi over every cell's faces),
// extrema with their cells, the first non-finite cell, probes and patch totals of phi and of the net face terms QhdView::F.
//
// Three launches per sample, qgd_monitor.hip's shape: qhdMonitorCellKernel (one partial row per workgroup), qhdMonitorPatchKernel (one
// partial row per chunk of a patch's face list), qhdMonitorFoldKernel<<<1, 256>>> (folds both, gathers the probes, writes the result
// block).  No float atomics, no in-launch ticket: lane l of workgroup b takes cells b * 256 + l, + grid * 256, ... in ascending label
// order; a cell's d_c is summed in its face list's order (ascending face label); lanes, waves, workgroups and chunks are folded in fixed
// trees.  Two samples of one state are bitwise equal.  Nothing here writes to the case.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "qgd_device.hpp"
#include "qgd_monitor_dev.hpp"   // the row stores, the folds and the "none" rules every block shares
#include "qgd_qhd_dev.hpp"       // QhdBdFrc: the body force as the step kernels form it

namespace qgd {

namespace {
typedef double mon2d __attribute__((ext_vector_type(2)));
constexpr MonitorShape SH = kQhdMonitorShape;
}

// ---- cells -------------------------------------------------------------------------------------------------------------------------
// row of SH.cellRow() doubles per workgroup: 12 sums | 4 x {min, label, max, label} | non-finite count, lowest label
// ROT: the case rotates (QhdBdFrc<QHD_ROT>); FLUX: a step has run, phi holds the flux of the last pressure solve
template <int ROT, bool FLUX>
__global__ __launch_bounds__(QGD_MON_BLOCK) void qhdMonitorCellKernel(const MonitorView mv, const MeshView m, const QhdView q) {
    __shared__ double sh[8];
    double s[SH.sums];
#pragma unroll
    for (int k = 0; k < SH.sums; ++k) s[k] = 0.0;
    ArgVal lo[SH.extrema], hi[SH.extrema];
    noExtrema(lo, hi);
    double bad = 0.0, badLabel = QGD_MON_NOLABEL;
    const mon2d* const c4 = reinterpret_cast<const mon2d*>(q.c4);
    const int64_t stride = (int64_t)gridDim.x * QGD_MON_BLOCK;
    for (int64_t i = (int64_t)mv.ownedBegin + (int64_t)blockIdx.x * QGD_MON_BLOCK + threadIdx.x; i < mv.ownedEnd; i += stride) {
        // everything that depends on the label alone is requested first: the record, p, V, the face count and the first eight face items
        const mon2d r0 = c4[2 * i], r1 = c4[2 * i + 1];
        const double p = q.p[i], V = m.V[i];
        const double label = mv.cellGlobal ? (double)mv.cellGlobal[i] : (double)(i + mv.cellGlobalOffset);
        double d = 0.0;
        if (FLUX) {
            const int n = m.cfCount[i];
            const size_t base = (size_t)m.cfSlice[i >> 6] * 64 + (size_t)(i & 63);
            for (int i0 = 0; i0 < n; i0 += 8) {   // eight faces per pass: the items, then the eight gathers in flight before the ordered sum
                int it[8];
                double x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) it[u] = i0 + u < n ? m.cfItem[base + (size_t)(i0 + u) * 64] : 0;
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = i0 + u < n ? q.phi[it[u] >= 0 ? it[u] : ~it[u]] : 0.0;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (i0 + u < n) d = it[u] >= 0 ? d + x[u] : d - x[u];   // + where the cell owns the face
            }
        }
        const double u4[4] = {r0.x, r0.y, r1.x, r1.y};
        const QhdBdFrc<ROT> B(q, u4);
        const double u2 = u4[0] * u4[0] + u4[1] * u4[1] + u4[2] * u4[2];
        s[0] += V;
        s[1] += u4[0] * V;
        s[2] += u4[1] * V;
        s[3] += u4[2] * V;
        s[4] += u4[3] * V;
        s[5] += 0.5 * u2 * V;
        s[6] += p * V;
        s[7] += B[0] * V;
        s[8] += B[1] * V;
        s[9] += B[2] * V;
        s[10] += d;
        s[11] += fabs(d);
        if (!(isFiniteD(u4[0]) && isFiniteD(u4[1]) && isFiniteD(u4[2]) && isFiniteD(u4[3]) && isFiniteD(p))) {
            markNonFinite(bad, badLabel, label);
            continue;   // extrema are taken over the cells whose state is finite
        }
        const double val[SH.extrema] = {sqrt(u2), u4[3], p, fabs(d) / V};
#pragma unroll
        for (int k = 0; k < SH.extrema; ++k) keepFinite(lo[k], hi[k], val[k], label);
    }
    storeCellRow(s, lo, hi, bad, badLabel, mv.cellPart + (size_t)blockIdx.x * SH.cellRow(), sh);
}

// ---- patch faces -------------------------------------------------------------------------------------------------------------------
// one workgroup per chunk (<= 256 consecutive entries of the face list, all of one patch); row of SH.patchRow doubles:
// |Sf|, phi, the four net face terms (patch faces keep them at their label), p_b Sf
template <bool FLUX>
__global__ __launch_bounds__(QGD_MON_BLOCK) void qhdMonitorPatchKernel(const MonitorView mv, const MeshView m, const QhdView q) {
    __shared__ double sh[4];
    const int first = mv.chunkStart[blockIdx.x], n = mv.chunkStart[blockIdx.x + 1] - first;
    double s[SH.patchRow];
#pragma unroll
    for (int k = 0; k < SH.patchRow; ++k) s[k] = 0.0;
    if ((int)threadIdx.x < n) {
        const int b = mv.faceList[first + threadIdx.x];   // boundary face index
        const size_t f = (size_t)m.nIF + b;
        s[0] = m.magSf[f];
        if (FLUX) {
            s[1] = q.phi[f];
#pragma unroll
            for (int k = 0; k < 4; ++k) s[2 + k] = q.F[(size_t)k * m.nF + f];
        }
        const double pb = q.pb[b];
        s[6] = pb * m.Sx[f]; s[7] = pb * m.Sy[f]; s[8] = pb * m.Sz[f];
    }
    storePatchRow(s, mv.patchPart + (size_t)blockIdx.x * SH.patchRow, sh);
}

// ---- fold --------------------------------------------------------------------------------------------------------------------------
// header: owned cells, fluxState, probes, patches, non-finite cells, the first of them | deltaT, flags (1: rotating, 2: frozen T)
__global__ __launch_bounds__(QGD_MON_BLOCK) void qhdMonitorFoldKernel(const MonitorView mv, const QhdView q, const int nCellRows, const int fluxState,
                                                                     double* __restrict__ out) {
    __shared__ double sh[8];
    const int t = threadIdx.x;
    const double nan = __builtin_nan("");
    double* hd = out + mv.off[0];
    double* in = out + mv.off[1];
    for (int k = 0; k < SH.sums; ++k) {
        const double x = foldColumn<OpSum>(mv.cellPart, SH.cellRow(), k, 0, nCellRows, 0.0, sh);
        if (t == 0) in[k] = k >= 10 && fluxState == 0 ? nan : x;   // no pressure solve yet: phi holds nothing
    }
    double* ex = out + mv.off[2];
    for (int k = 0; k < SH.extrema; ++k) {
        const MinMax e = foldExtremum(mv.cellPart, SH.cellRow(), SH.sums + 4 * k, 0, nCellRows, sh);
        if (t == 0) storeExtremum(ex + 4 * k, e, k == 3 && fluxState == 0);   // no continuity error yet
    }
    const NonFinite nf = foldNonFinite(mv.cellPart, SH.cellRow(), SH.sums + 4 * SH.extrema, 0, nCellRows, sh);
    if (t == 0) {
        monitorHeader(hd, mv, fluxState, nf);
        hd[6] = q.dt;
        hd[7] = (double)((q.rotating ? 1 : 0) | (q.frozenT ? 2 : 0));
    }
    // probes: Ux, Uy, Uz, T, p
    double* pr = out + mv.off[3];
    for (int i = t; i < mv.nProbes; i += QGD_MON_BLOCK) {
        const int cell = mv.probeCell[i];
        double* o = pr + (size_t)i * SH.probeRow;
        if (cell < 0) {
#pragma unroll
            for (int k = 0; k < SH.probeRow; ++k) o[k] = nan;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = q.c4[(size_t)cell * 4 + k];
            o[4] = q.p[cell];
        }
    }
    // patches.  phi (column 1) -- fluxState 0: no step yet; the terms 2..5 -- 2: implicitDiffusion, where F holds the explicit part only; a
    // frozen T has no equation, so no flux
    const bool frozenT = q.frozenT;
    foldPatches(mv, mv.patchPart, SH.patchRow, out + mv.off[4], sh,
                [=](int k) { return (k == 1 && fluxState == 0) || (k >= 2 && k <= 5 && fluxState != 1) || (k == 5 && frozenT); });
}

void launchQhdMonitorSample(hipStream_t s, const MonitorView& mv, const MeshView& m, const QhdView& q, int fluxState, double* out) {
    const int64_t nOwned = (int64_t)mv.ownedEnd - mv.ownedBegin;
    const int grid = (int)std::min<int64_t>((nOwned + QGD_MON_BLOCK - 1) / QGD_MON_BLOCK, QGD_MONITOR_BLOCKS);
    const bool flux = fluxState != 0;
    if (grid > 0) {
        if (q.rotating) {
            if (flux) qhdMonitorCellKernel<QHD_ROT, true><<<grid, QGD_MON_BLOCK, 0, s>>>(mv, m, q);
            else qhdMonitorCellKernel<QHD_ROT, false><<<grid, QGD_MON_BLOCK, 0, s>>>(mv, m, q);
        } else {
            if (flux) qhdMonitorCellKernel<0, true><<<grid, QGD_MON_BLOCK, 0, s>>>(mv, m, q);
            else qhdMonitorCellKernel<0, false><<<grid, QGD_MON_BLOCK, 0, s>>>(mv, m, q);
        }
    }
    if (mv.nChunks > 0) {
        if (flux) qhdMonitorPatchKernel<true><<<mv.nChunks, QGD_MON_BLOCK, 0, s>>>(mv, m, q);
        else qhdMonitorPatchKernel<false><<<mv.nChunks, QGD_MON_BLOCK, 0, s>>>(mv, m, q);
    }
    qhdMonitorFoldKernel<<<1, QGD_MON_BLOCK, 0, s>>>(mv, q, grid, fluxState, out);
}

}  // namespace qgd
