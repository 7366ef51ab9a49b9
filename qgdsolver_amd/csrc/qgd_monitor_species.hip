// qgd_monitor_species.hip -- the species block of a run monitor (gfx950, wave64; qgd_monitor_enable_species of include/qgd_amd.h): per
// species of a case that carries species (qgd_species.hip), the inert one included, sum rho Y_i V over the owned cells, {min, its cell,
// max, its cell} of Y_i, Y_i at the monitor's probe cells and, per requested patch, the total of the net species flux the species cell
// update consumed; with them the count and first label of cells with a non-finite Y_i and max |sum_i Y_i - 1|.
//
// Three launches per sample whatever nS is, behind the flow block's three (qgd_monitor.hip), under its rules -- no float atomics, no
// in-launch ticket, nothing written to the case, every sum folded in an order that depends on the mesh, the specification and nS only:
//   monitorSpeciesCellKernel   the owned range in tiles of 1024 cells, workgroup b takes the tiles b, b + grid, ... (at most
//                              QGD_MONITOR_BLOCKS workgroups), lane l the four cells l + {0, 256, 512, 768} of a tile
//                              (QGD_MONITOR_SPECIES_CELLS); rho, V and the labels of its cells stay in registers while the species-major
//                              planes Y[i * nC + cell] go by ONCE, coalesced, in register batches of QGD_SPECIES_W species -- per lane a
//                              batch holds four sums and four {min, label, max, label} sets; the per-cell sum of all Y_i and the
//                              non-finite mask ride along the batches.  One partial row per workgroup.
//   monitorSpeciesPatchKernel  one workgroup per chunk of the monitor's face list (<= 256 faces of one patch), one partial row per chunk
//   monitorSpeciesFoldKernel   <<<1, 256>>>: folds both (thread t takes rows t, t + 256, ... in ascending order, then the block tree),
//                              gathers the probes, writes the species block
// Ghost cells of a shard and the copies behind cyclic halves lie outside [ownedBegin, ownedEnd); the face list holds no face they own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "qgd_device.hpp"

#include "../../include/qgd_amd.h"
#include "qgd_monitor_dev.hpp"
#include "qgd_species_dev.hpp"

namespace qgd {

// ---- cells -------------------------------------------------------------------------------------------------------------------------
// row of 5 nS + 3 doubles per workgroup: nS sums of (rho Y_i) V | nS x {min, label, max, label} | cells with a non-finite Y_i, the lowest
// label among them, max |sum_i Y_i - 1| over the cells whose Y_i are all finite (-1: no such cell).
// A tile is 256 * K consecutive owned cells; workgroup b takes the tiles b, b + grid, ... in ascending order.  Within a tile the lanes fold
// a batch's sums and extrema across their wave by shuffles (no barrier) and lane 0 adds the result to its wave's own accumulators in LDS;
// the four waves' accumulators are combined in wave order at the end.
template <int W, int K>
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorSpeciesCellKernel(const MonitorView mv, const SpeciesMonitorView sm, const MeshView m, const CaseView c,
                                                                         const SpeciesView sv, const int nTiles) {
    __shared__ double sh[8];
    __shared__ double acc[4][5 * QGD_MAX_SPECIES_DEV];   // per wave: nS sums | nS x {min, label, max, label}
    const size_t nC = (size_t)m.nC;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nS = sv.nS;
    for (int i = lane; i < nS; i += 64) {
        acc[wave][i] = 0.0;
        double* e = &acc[wave][nS + 4 * i];
        e[0] = INFINITY; e[1] = QGD_MON_NOLABEL; e[2] = -INFINITY; e[3] = QGD_MON_NOLABEL;
    }
    __syncthreads();
    double nb = 0.0, lb = QGD_MON_NOLABEL, defect = -1.0;
    for (int tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const int64_t base = (int64_t)mv.ownedBegin + (int64_t)tile * (QGD_MON_BLOCK * K) + threadIdx.x;
        int64_t cell[K];
        double rho[K], V[K], label[K], ysum[K];
        unsigned on = 0, bad = 0;   // bit j: cell j of this lane is an owned cell | has a non-finite Y_i
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int64_t i = base + (int64_t)j * QGD_MON_BLOCK;
            if (i < mv.ownedEnd) on |= 1u << j;
            cell[j] = i < mv.ownedEnd ? i : (int64_t)mv.ownedEnd - 1;   // (a lane past the range re-reads the last owned cell and counts nothing)
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            rho[j] = c.A[cell[j]].rho;
            V[j] = m.V[cell[j]];
            label[j] = mv.cellGlobal ? (double)mv.cellGlobal[cell[j]] : (double)(cell[j] + mv.cellGlobalOffset);
            ysum[j] = 0.0;
        }
        for (int s0 = 0; s0 < nS; s0 += W) {
            double y[W][K];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const double* __restrict__ Y = sv.Y + (size_t)min(s0 + k, nS - 1) * nC;   // (slots past the last species repeat it and store nothing)
#pragma unroll
                for (int j = 0; j < K; ++j) y[k][j] = Y[cell[j]];
            }
            double s[W];
            ArgVal lo[W], hi[W];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                s[k] = 0.0;
                lo[k] = noMin();
                hi[k] = noMax();
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (!(on >> j & 1u) || s0 + k >= nS) continue;
                    const double v = y[k][j];
                    s[k] += (rho[j] * v) * V[j];
                    ysum[j] += v;
                    if (!isFiniteD(v)) { bad |= 1u << j; continue; }   // the extrema of a species are taken over the cells where it is finite
                    keepExtrema(lo[k], hi[k], v, label[j]);
                }
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (s0 + k >= nS) continue;   // (the same for every lane)
                const double r = waveFold<OpSum>(s[k]);
                const ArgVal a = waveFoldArg<false>(lo[k]);
                const ArgVal b = waveFoldArg<true>(hi[k]);
                if (lane == 0) {              // the wave's own accumulators: no other wave touches them before the barrier below
                    acc[wave][s0 + k] += r;
                    double* e = &acc[wave][nS + 4 * (s0 + k)];
                    const ArgVal a1 = argMin(ArgVal{e[0], e[1]}, a), b1 = argMax(ArgVal{e[2], e[3]}, b);
                    e[0] = a1.v; e[1] = a1.l; e[2] = b1.v; e[3] = b1.l;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (!(on >> j & 1u)) continue;
            if (bad >> j & 1u) { nb += 1.0; lb = fmin(lb, label[j]); }
            else defect = fmax(defect, fabs(ysum[j] - 1.0));
        }
    }
    __syncthreads();
    double* row = sm.cellPart + (size_t)blockIdx.x * (5 * (size_t)nS + 3);
    for (int i = threadIdx.x; i < nS; i += QGD_MON_BLOCK) {
        row[i] = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
        ArgVal a{acc[0][nS + 4 * i], acc[0][nS + 4 * i + 1]}, b{acc[0][nS + 4 * i + 2], acc[0][nS + 4 * i + 3]};
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const double* e = &acc[w][nS + 4 * i];
            a = argMin(a, ArgVal{e[0], e[1]});
            b = argMax(b, ArgVal{e[2], e[3]});
        }
        double* e = row + nS + 4 * i;
        e[0] = a.v; e[1] = a.l; e[2] = b.v; e[3] = b.l;
    }
    nb = blockFold<OpSum>(nb, sh);
    lb = blockFold<OpMin>(lb, sh);
    defect = blockFold<OpMax>(defect, sh);
    if (threadIdx.x == 0) { double* e = row + 5 * (size_t)nS; e[0] = nb; e[1] = lb; e[2] = defect; }
}

// ---- patch faces -------------------------------------------------------------------------------------------------------------------
// one workgroup per chunk; row of nS doubles: the net flux of every species out of the domain through the chunk's faces, as the species'
// cell update consumed it.  Explicit branch: SpeciesView::F at the face's position (a patch face keeps its label).  Implicit branch
// (aF != nullptr): F holds phiJmY_i alone; the diffusive part is YEqn.flux() on the face as caseSpeciesImplFluxKernel forms it,
// -(a_b / Sc_i)(Y_b - Y_P) with the new Y_i of the owner, on the faces of the species' fixedValue patches and zero elsewhere.  The inert
// species: phiJm of the face minus the transported species' fluxes, what Y_inert = 1 - sum implies.
template <int W>
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorSpeciesPatchKernel(const MonitorView mv, const SpeciesMonitorView sm, const MeshView m, const CaseView c,
                                                                          const SpeciesView sv, const double* __restrict__ aF) {
    __shared__ double sh[4];
    const int first = mv.chunkStart[blockIdx.x], n = mv.chunkStart[blockIdx.x + 1] - first;
    const bool on = (int)threadIdx.x < n;
    const size_t nC = (size_t)m.nC, nF = (size_t)m.nF;
    const int b = on ? mv.faceList[first + threadIdx.x] : 0;   // boundary face index
    const size_t f = (size_t)m.nIF + b;
    const int own = on ? m.own[f] : 0, patch = on ? m.bPatch[b] : 0;
    const double a = (on && aF) ? aF[f] : 0.0;
    double inert = on ? c.flux[f] : 0.0;
    double* row = sm.patchPart + (size_t)blockIdx.x * sv.nS;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) {
        int sp[W];
        double x[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int slot = min(a0 + k, sv.nAct - 1);
            sp[k] = sv.act[slot];
            x[k] = on ? sv.F[(size_t)slot * nF + f] : 0.0;
            if (on && aF) {
                const size_t e = (size_t)sp[k] * sv.nPatches + patch;
                if (sv.bcKind[e] == QGD_BC_FIXEDVALUE) x[k] += -((a / sv.Sc[sp[k]]) * (sv.bcVal[e] - sv.Y[(size_t)sp[k] * nC + own]));
            }
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (a0 + k >= sv.nAct) continue;   // (the same for every lane of the workgroup)
            inert -= x[k];
            const double r = blockFold<OpSum>(x[k], sh);
            if (threadIdx.x == 0) row[sp[k]] = r;
        }
    }
    const double r = blockFold<OpSum>(inert, sh);
    if (threadIdx.x == 0) row[sv.inert] = r;
}

// ---- fold --------------------------------------------------------------------------------------------------------------------------
// header: nS, the inert species, fluxState, cells with a non-finite Y_i, the first of them, max |sum_i Y_i - 1|, probes, patches
__global__ __launch_bounds__(QGD_MON_BLOCK) void monitorSpeciesFoldKernel(const MonitorView mv, const SpeciesMonitorView sm, const SpeciesView sv, const int nC,
                                                                         const int fluxState, double* __restrict__ out) {
    __shared__ double sh[8];
    const int t = threadIdx.x, nS = sv.nS;
    const size_t rowLen = 5 * (size_t)nS + 3;
    const double nan = __builtin_nan("");
    double* hd = out + sm.off[0];
    double* in = out + sm.off[1];
    double* ex = out + sm.off[2];
    for (int i = 0; i < nS; ++i) {
        const double x = foldColumn<OpSum>(sm.cellPart, rowLen, i, 0, sm.nRows, 0.0, sh);
        const MinMax e = foldExtremum(sm.cellPart, rowLen, nS + 4 * i, 0, sm.nRows, sh);
        if (t == 0) { in[i] = x; storeExtremum(ex + 4 * i, e, false); }
    }
    const NonFinite nf = foldNonFinite(sm.cellPart, rowLen, 5 * nS, 0, sm.nRows, sh);
    const double defect = foldColumn<OpMax>(sm.cellPart, rowLen, 5 * nS + 2, 0, sm.nRows, -1.0, sh);
    if (t == 0) {
        hd[0] = (double)nS;
        hd[1] = (double)sv.inert;
        hd[2] = (double)fluxState;
        hd[3] = nf.count;
        hd[4] = nf.first();
        hd[5] = defect < 0.0 ? nan : defect;   // no owned cell whose Y_i are all finite
        hd[6] = (double)mv.nProbes;
        hd[7] = (double)mv.nPatches;
    }
    // probes: Y_i of the probe's cell, all species
    double* pr = out + sm.off[3];
    for (int i = t; i < mv.nProbes; i += QGD_MON_BLOCK) {
        const int cell = mv.probeCell[i];
        for (int k = 0; k < nS; ++k) pr[(size_t)i * nS + k] = cell < 0 ? nan : sv.Y[(size_t)k * nC + cell];
    }
    // patches: every column NaN while nothing is assembled yet
    foldPatches(mv, sm.patchPart, nS, out + sm.off[4], sh, [=](int) { return fluxState == 0; });
}

void launchMonitorSpeciesSample(hipStream_t s, const MonitorView& mv, const SpeciesMonitorView& sm, const MeshView& m, const CaseView& c,
                                const SpeciesView& sv, const double* aF, int fluxState, double* out) {
    constexpr int W = QGD_SPECIES_W, K = QGD_MONITOR_SPECIES_CELLS;
    const int64_t nOwned = (int64_t)mv.ownedEnd - mv.ownedBegin, tile = (int64_t)QGD_MON_BLOCK * K;
    const int nTiles = (int)((nOwned + tile - 1) / tile);   // sm.nRows = min(nTiles, QGD_MONITOR_BLOCKS) workgroups
    if (sm.nRows > 0) monitorSpeciesCellKernel<W, K><<<sm.nRows, QGD_MON_BLOCK, 0, s>>>(mv, sm, m, c, sv, nTiles);
    if (mv.nChunks > 0) monitorSpeciesPatchKernel<W><<<mv.nChunks, QGD_MON_BLOCK, 0, s>>>(mv, sm, m, c, sv, fluxState == 2 ? aF : nullptr);
    monitorSpeciesFoldKernel<<<1, QGD_MON_BLOCK, 0, s>>>(mv, sm, sv, m.nC, fluxState, out);
}

}  // namespace qgd
