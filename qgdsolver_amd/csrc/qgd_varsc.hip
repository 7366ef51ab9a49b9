// qgd_varsc.hip -- the varScModel7 closure of QGDCoeffs (gfx950): ScQGD per cell from the pressure jumps across the cell's faces
// [varScModel7_8C_source.html L166-300].  tau, tauQGDf and alphauQGD stay those of constScPrModel1 [L173-174, L277-300]; the kernels
// that form muQGD = p ScQGD tauQGD read the array this one writes (CaseView::sc).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/qgd_amd.h"
#include "qgd_device.hpp"
#include "qgd_stencil_dev.hpp"

namespace qgd {

namespace {

// One lane per cell, ghosts excepted (a shard's ghost cells lack faces; their muQGD arrives by message).  The cell's faces come through
// the slot-major cell-face tables of the cell kernels (cfItem: the face label, ~label where the cell is the face's neighbour; cfNbr: the cell
// across, -1 on a patch face), eight per pass with every load of a pass requested before the first use (cellGradGauss).
//   internal face:  sumpf += lin(p)_f,  sumDpF += r_f (p_other - p_self)   [L187-207: +dpf for the owner, -dpf for the neighbour]
//   patch face:     sumpf += p_b,       sumDpF += r_b (p_b - p_self)       [L209-232], none of either on an empty patch (rf < 0)
//   ScQGD = cSc1 |sumDpF| / (sumpf / n), clipped to [minSc, maxSc] where those are >= 0 [L234-244], constSc on constScCellSet [L246-254]
// p_b is the patch pressure the muQGD lines of the boundary refresh read (bPmid: after GaussVolPoint's mid-assembly evaluation of a
// qgdFlux wall; the boundary refresh leaves the new patch pressure there, so it serves start-up as well).
// init (createFields.H builds the thermo object, which runs the model once): muQGD of the record follows the new ScQGD.
__global__ __launch_bounds__(QGD_BLOCK) void varSc7Kernel(const MeshView m, const CaseView c, const GasModel gm, const VarScView v, const int init) {
    const int ci = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (ci >= m.nC) return;
    if (m.ghost && m.ghost[ci] == 1) return;
    const int n = m.cfCount[ci];
    const size_t base = (size_t)m.cfSlice[ci >> 6] * 64 + (ci & 63);
    const double pc = c.A[ci].p;
    double sumDp = 0.0, sumP = 0.0;
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 8) {
        int it[8], nb[8];
        double w[8], r[8], pn[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool on = i0 + u < n;
            it[u] = on ? m.cfItem[base + (size_t)(i0 + u) * 64] : 0;
            nb[u] = on ? m.cfNbr[base + (size_t)(i0 + u) * 64] : -1;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool on = i0 + u < n;
            const int f = it[u] >= 0 ? it[u] : ~it[u];
            r[u] = on ? v.rf[f] : -1.0;   // r < 0: skipped like the face of an empty patch
            w[u] = on ? m.w[f] : 0.0;
            pn[u] = nb[u] >= 0 ? c.A[nb[u]].p : ((on && f >= m.nIF) ? c.bPmid[f - m.nIF] : pc);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (r[u] < 0.0) continue;
            const double pf = nb[u] < 0 ? pn[u] : (it[u] >= 0 ? lerpf(w[u], pc, pn[u]) : lerpf(w[u], pn[u], pc));   // lerp(w, owner, neighbour)
            sumP += pf;
            sumDp += r[u] * (pn[u] - pc);
            ++cnt;
        }
    }
    double sc = v.cSc1 * fabs(sumDp) / (sumP / (double)cnt);
    if (v.minSc >= 0.0) sc = fmax(sc, v.minSc);
    if (v.maxSc >= 0.0) sc = fmin(sc, v.maxSc);
    if (v.constCell && v.constCell[ci]) sc = v.ScQGD;
    v.sc[ci] = sc;
    if (init) {
        const double aq = c.aQ ? c.aQ[ci] : gm.alphaQGD;
        const double tauQGD = aq * m.hQGD[ci] / c.B[ci].c;
        c.B[ci].muQGD = pc * sc * tauQGD;
    }
}

// max / min ScQGD over cells [begin, end): per-workgroup partials, then one workgroup
__global__ __launch_bounds__(QGD_BLOCK) void varScRangeKernel(const VarScView v, const int begin, const int end, const int stage, const int nPartials) {
    double hi = -1e300, lo = 1e300;
    if (stage == 0) {
        for (int i = begin + blockIdx.x * QGD_BLOCK + threadIdx.x; i < end; i += gridDim.x * QGD_BLOCK) {
            const double s = v.sc[i];
            hi = fmax(hi, s); lo = fmin(lo, s);
        }
        blockMaxMin(hi, lo, v.part + 2 * (size_t)blockIdx.x, false);
    } else {
        for (int i = threadIdx.x; i < nPartials; i += QGD_BLOCK) {
            hi = fmax(hi, v.part[2 * (size_t)i]); lo = fmin(lo, v.part[2 * (size_t)i + 1]);
        }
        blockMaxMin(hi, lo, v.part + 2 * (size_t)QGD_FACE_REDUCE_PARTIALS, false);
    }
}

}  // namespace

void launchVarSc7(const Launcher& L, const MeshView& m, const CaseView& c, const GasModel& g, const VarScView& v, bool init) {
    if (m.nC == 0) return;
    if (L.pre) L.pre(L.ctx, QGD_K_VARSC);
    varSc7Kernel<<<(m.nC + QGD_BLOCK - 1) / QGD_BLOCK, QGD_BLOCK, 0, L.stream>>>(m, c, g, v, init ? 1 : 0);
    if (L.post) L.post(L.ctx, QGD_K_VARSC);
}

void launchVarScRange(hipStream_t s, const VarScView& v, int32_t begin, int32_t end) {
    const int n = std::max(end - begin, 0);
    const int blocks = std::max(1, std::min((n + QGD_BLOCK - 1) / QGD_BLOCK, QGD_FACE_REDUCE_PARTIALS));
    varScRangeKernel<<<blocks, QGD_BLOCK, 0, s>>>(v, begin, end, 0, 0);
    varScRangeKernel<<<1, QGD_BLOCK, 0, s>>>(v, begin, end, 1, blocks);
}

}  // namespace qgd
