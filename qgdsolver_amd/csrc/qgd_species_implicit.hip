// qgd_species_implicit.hip -- the species block of a resident QGDFoam case on the implicitDiffusion branch (gfx950 / CDNA4, wave64):
//     fvm::ddt(rho, Yi) + fvc::div(phiJmYi) - fvm::laplacian(muf/ScNumbers[i], Yi);  diffusiveFlux[i] += YEqn.flux()     [QGDYEqn.H L47-66]
// the reference's default (QGDThermo::read gives implicitDiffusion true when the entry is absent).  Runs inside the implicit advance of
// qgd_case_step, after deltaT and before the U systems, on the records of the state before the step; passive composition, as qgd_species.hip.
//
//   SP        the vertex values (qgd_species.hip)
//   SF / SFB  caseSpeciesImplFaceKernel / caseSpeciesImplBoundaryFaceKernel<ST, W>: the explicit branch's face walks with speciesBatch's
//             IMPL flag: phiJmY_i alone at the face's position, a_f = muf |Sf| delta_f once per face
//   SA        caseSpeciesImplCellKernel<W>: the rows of a register batch, one lane per cell
//   solve     ONE per batch: implicitSolveSetup(S, nRhs <= 4, ..., gam[k] = 1/Sc_k) on the case's ImplicitSolver (Chebyshev; QGD_IMPL_SOLVER=pcg:
//             conjugate gradients) -- one matrix walk per iteration for the whole batch instead of one per species
//   SX        caseSpeciesImplFluxKernel<W>: YEqn.flux() of the new Y_i, the inert species' diffusiveFlux (QGD_SPECIES_KEEP_FLUXES only)
//   SM        caseSpeciesImplClipKernel<W>: Yi.max(0), Y_inert = max(1 - sum, 0); then the patch values (qgd_species.hip)
// The block reads plane 0 of CaseView::flux on every face: a case with species assembles the U systems with the separate kernels, not
// block-fused (fusedFaceCellKernel<..., IMPL> keeps the internal faces' mass flux in its blocks); qgd_case_fused_info reports 0.
// The solves start from the old Y_i (OpenFOAM's start value): the time-extrapolated start values of the flow's solves (QGD_IMPL_XEXTRAP)
// are not extended to the species.
#include "qgd_device.hpp"

#include <algorithm>

#include "../../include/qgd_amd.h"
#include "qgd_species_dev.hpp"
#include "qgd_stencil_dev.hpp"

namespace qgd {

// The same two walks for the implicitDiffusion branch [QGDYEqn.H L47-66] (speciesBatch<..., IMPL = true>): phiJmY_i alone goes to the face's
// position, and the species-independent laplacian coefficient a_f = muf |Sf| delta_f to aF, once per face.  Kernels of their own, in a file of their own: the
// explicit ones stay what they were instruction for instruction (scripts/kernel_resources.py --compare).
template <int ST, int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesImplFaceKernel(const MeshView m, const CaseView c, const GasModel gm, const SpeciesView sv,
                                                                      const SpeciesImplView iv) {
    const int f = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (f >= m.nIF) return;
    const size_t pos = (size_t)m.fpos[f];
    SpeciesFace F;
    F.o = m.own[f]; F.n = m.nei[f];
    F.w = m.w[f]; F.dn = m.dn[f];
    const double hf = m.hf[f], ms = m.magSf[f];
    const double S[3] = {m.Sx[f], m.Sy[f], m.Sz[f]};
    F.phiJm = c.flux[pos];
    const RecA Ao = c.A[F.o], An = c.A[F.n];
    const RecB Bo = c.B[F.o], Bn = c.B[F.n];
    const double Uo[3] = {Ao.ux, Ao.uy, Ao.uz}, Un[3] = {An.ux, An.uy, An.uz};
    double phi = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F.Uf[k] = lerpf(F.w, Uo[k], Un[k]);
        phi += S[k] * lerpf(F.w, Ao.rho * Uo[k], An.rho * Un[k]);   // phi = Sf & lin(rho U)
    }
    F.phiTau = phi * (lerpf(F.w, Bo.aOc, Bn.aOc) * hf);             // tauQGDf = lin(alphaQGD / c) hQGDf [constScPrModel1_8C L103]
    F.mufS = lerpf(F.w, muEffOf(gm, Bo.muQGD), muEffOf(gm, Bn.muQGD)) * ms;
    iv.aF[pos] = F.mufS * F.dn;
    double inertDf = 0.0;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) speciesBatch<ST, W, true, true>(m, sv, F, f, pos, a0, inertDf);
    if (sv.phiJmY) sv.phiJmY[(size_t)sv.inert * m.nF + f] = 0.0;   // (the inert diffusiveFlux: caseSpeciesImplFluxKernel, after the solves)
}
template <int ST, int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesImplBoundaryFaceKernel(const MeshView m, const CaseView c, const GasModel gm, const SpeciesView sv,
                                                                              const SpeciesImplView iv) {
    const int b = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (b >= m.nBF) return;
    const int f = m.nIF + b;
    const size_t nF = (size_t)m.nF;
    if (m.fkind[f] == 3) {   // empty patches carry no field
        for (int a = 0; a < sv.nAct; ++a) sv.F[(size_t)a * nF + f] = 0.0;
        iv.aF[f] = 0.0;
        if (sv.phiJmY)
            for (int i = 0; i < sv.nS; ++i) { sv.phiJmY[(size_t)i * nF + f] = 0.0; sv.dflux[(size_t)i * nF + f] = 0.0; }
        return;
    }
    SpeciesFace F;
    F.o = m.own[f]; F.n = b;
    F.w = 1.0; F.dn = m.dn[f];
    const double hf = m.hf[f], ms = m.magSf[f];
    const double S[3] = {m.Sx[f], m.Sy[f], m.Sz[f]};
    F.phiJm = c.flux[f];
    const RecA Ab = c.bA[b];
    const RecB Bb = c.bB[b];
    const double Ub[3] = {Ab.ux, Ab.uy, Ab.uz}, rhoLag = c.bRhoLag[b];
    double phi = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { F.Uf[k] = Ub[k]; phi += S[k] * (rhoLag * Ub[k]); }   // rhoU_b [QGDUEqn_8H L88-89]
    F.phiTau = phi * (Bb.aOc * hf);
    F.mufS = muEffOf(gm, Bb.muQGD) * ms;
    iv.aF[f] = F.mufS * F.dn;
    double inertDf = 0.0;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) speciesBatch<ST, W, false, true>(m, sv, F, f, (size_t)f, a0, inertDf);
    if (sv.phiJmY) sv.phiJmY[(size_t)sv.inert * nF + f] = 0.0;
}

// ---- the implicitDiffusion branch [QGDYEqn.H L47-66]: fvm::ddt(rho, Yi) + fvc::div(phiJmYi) - fvm::laplacian(muf/Sc_i, Yi) ------------------
// All species share a_f = muf |Sf| delta_f (SpeciesImplView::aF, by position) and differ by 1/Sc_i only: a register batch is ONE solve with
// up to W right-hand sides whose face coefficients are gam[k] a_f, gam[k] = 1/Sc_k (ISolveView::gam).
//
// SA  rows of the species a0 .. a0 + W - 1 of one cell, one lane per cell over the cell -> face table, no atomics; the list entries of
//     eight faces are requested before the first gather (as iApplyKernel):
//         diag = rho V/dt + (1/Sc_i) (sum a_f over internal faces + sum a_b over the species' fixedValue patch faces)
//         rhs  = rho.old Y_i V/dt - sum +-phiJmY_i + (1/Sc_i) sum a_b Y_b      (fvc::surfaceIntegrate: ascending face label)
//         x    = Y_i                                                          (OpenFOAM's start value)
//     rho from the same mass fluxes and deltaT as caseSpeciesCellKernel forms it.  Components past the last species (nr > the species left)
//     get the row 1 x = 0; the solve's valid mask leaves them out.
template <int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesImplCellKernel(const MeshView m, const CaseView c, const SpeciesView sv, const SpeciesImplView iv,
                                                                      const int a0, const int nr) {
    const int ci = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (ci >= m.nC) return;
    const int n = m.cfCount[ci];
    const size_t base = (size_t)m.cfSlice[ci >> 6] * 64 + (ci & 63);
    const size_t nC = (size_t)m.nC, nF = (size_t)m.nF;
    int sp[W], slot[W];
    double s[W], dB[W], sB[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { slot[k] = min(a0 + k, sv.nAct - 1); sp[k] = sv.act[slot[k]]; s[k] = dB[k] = sB[k] = 0.0; }
    double sum0 = 0.0, dsum = 0.0;
    constexpr int U = 8;
    for (int e0 = 0; e0 < n; e0 += U) {
        int it[U];
        double fx[U], ax[U], Fx[W][U];
#pragma unroll
        for (int u = 0; u < U; ++u) it[u] = e0 + u < n ? m.cfPos[base + (size_t)(e0 + u) * 64] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = e0 + u < n;
            const size_t pos = (size_t)(it[u] >= 0 ? it[u] : ~it[u]);
            fx[u] = on ? c.flux[pos] : 0.0;
            ax[u] = on ? iv.aF[pos] : 0.0;
#pragma unroll
            for (int k = 0; k < W; ++k) Fx[k][u] = on ? sv.F[(size_t)slot[k] * nF + pos] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (e0 + u >= n) continue;
            const int pos = it[u] >= 0 ? it[u] : ~it[u];
            sum0 = it[u] >= 0 ? sum0 + fx[u] : sum0 - fx[u];
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] = it[u] >= 0 ? s[k] + Fx[k][u] : s[k] - Fx[k][u];
            if (pos < m.nIF) dsum += ax[u];
            else {   // a patch face keeps its label: fixedValue adds a_b to the diagonal and a_b Y_b to the source, anything else nothing
                const int patch = m.bPatch[pos - m.nIF];
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const size_t e = (size_t)sp[k] * sv.nPatches + patch;
                    if (sv.bcKind[e] == QGD_BC_FIXEDVALUE) { dB[k] += ax[u]; sB[k] += ax[u] * sv.bcVal[e]; }
                }
            }
        }
    }
    const double V = m.V[ci], dt = c.dt[0];
    const double rhoOld = c.A[ci].rho;
    const double dtV = dt / V;
    const double rhoNew = rhoOld - dtV * sum0;                                   // [QGDRhoEqn_8H L40-47]
    const double rDeltaT = 1.0 / dt;
    const double den = rDeltaT * rhoNew * V;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if (k >= nr) continue;
        const size_t j = (size_t)k * nC + ci, jx = (size_t)(a0 + k) * nC + ci;
        if (a0 + k < sv.nAct) {
            const double gam = 1.0 / sv.Sc[sp[k]], y = sv.Y[(size_t)sp[k] * nC + ci];
            iv.diag[j] = den + gam * (dsum + dB[k]);
            iv.rhs[j] = (rDeltaT * rhoOld * y * V - s[k]) + gam * sB[k];
            iv.x[jx] = y;
        } else { iv.diag[j] = 1.0; iv.rhs[j] = 0.0; iv.x[jx] = 0.0; }
    }
}

// SX  diffusiveFlux_i += YEqn.flux() of the NEW Y_i [L64]: -(a_f/Sc_i)(Y_N - Y_O) inside, -(a_b/Sc_i)(Y_b - Y_P) on fixedValue faces -- the
//     sign "- fvm::laplacian" gives it, opposite to the explicit branch's; as listed.  Then diffusiveFlux_inert -= diffusiveFlux_i, the running
//     total [L65].  QGD_SPECIES_KEEP_FLUXES only (nothing else reads diffusiveFlux).
template <int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesImplFluxKernel(const MeshView m, const SpeciesView sv, const SpeciesImplView iv) {
    const int f = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (f >= m.nF) return;
    if (m.fkind[f] == 3) return;   // (cleared by the face kernel)
    const bool internal = f < m.nIF;
    const size_t nC = (size_t)m.nC, nF = (size_t)m.nF;
    const double a = iv.aF[internal ? (size_t)m.fpos[f] : (size_t)f];
    const int o = m.own[f], nb = internal ? m.nei[f] : o;
    const int patch = internal ? 0 : m.bPatch[f - m.nIF];
    double inertDf = 0.0;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) {
        int sp[W];
        double xo[W], xn[W], df[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int sl = min(a0 + k, sv.nAct - 1);
            sp[k] = sv.act[sl];
            xo[k] = iv.x[(size_t)sl * nC + o];
            xn[k] = iv.x[(size_t)sl * nC + nb];
            df[k] = sv.dflux[(size_t)sp[k] * nF + f];
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (a0 + k >= sv.nAct) continue;
            double fl = 0.0;
            if (internal) fl = -((a / sv.Sc[sp[k]]) * (xn[k] - xo[k]));
            else {
                const size_t e = (size_t)sp[k] * sv.nPatches + patch;
                if (sv.bcKind[e] == QGD_BC_FIXEDVALUE) fl = -((a / sv.Sc[sp[k]]) * (sv.bcVal[e] - xo[k]));
            }
            const double d = df[k] + fl;
            sv.dflux[(size_t)sp[k] * nF + f] = d;
            inertDf -= d;
        }
    }
    sv.dflux[(size_t)sv.inert * nF + f] = inertDf;
}

// SM  Yi.max(0) [L86], Y_inert = max(1 - sum, 0) [L90-91] from the solutions
template <int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesImplClipKernel(const MeshView m, const SpeciesView sv, const SpeciesImplView iv) {
    const int ci = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (ci >= m.nC) return;
    const size_t nC = (size_t)m.nC;
    double Yt = 0.0;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) {
        double x[W];
#pragma unroll
        for (int k = 0; k < W; ++k) x[k] = iv.x[(size_t)min(a0 + k, sv.nAct - 1) * nC + ci];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (a0 + k >= sv.nAct) continue;
            const double yn = fmax(x[k], 0.0);
            sv.Y[(size_t)sv.act[a0 + k] * nC + ci] = yn;
            Yt += yn;
        }
    }
    sv.Y[(size_t)sv.inert * nC + ci] = fmax(1.0 - Yt, 0.0);
}

// the implicitDiffusion branch: fluxes and a_f of the old state, then per batch of W species the rows, ONE solve with gam[k] = 1/Sc_k
// (Chebyshev or conjugate gradients, as the flow's solves; start value Y_i: the flow's time-extrapolated start values, QGD_IMPL_XEXTRAP,
// are not extended to the species), its statistics into `stats` (slot = batch); last YEqn.flux(), the clip, the inert species, patch values
template <int ST>
static void launchSpeciesAdvanceImplicitT(hipStream_t s, const MeshView& m, const CaseView& c, const GasModel& g, const SpeciesView& sv,
                                          const SpeciesImplView& iv, ImplicitSolver* S, double tol, int maxIter, double* stats) {
    constexpr int W = QGD_SPECIES_W;
    static_assert(W <= 4, "a batch is one solve of the implicit solver: at most four right-hand sides");
    if (ST == ST_GVP3 || ST == ST_GVP2) launchSpeciesPoints(s, m, sv);
    if (m.nIF) caseSpeciesImplFaceKernel<ST, W><<<gridOfS(m.nIF), QGD_BLOCK, 0, s>>>(m, c, g, sv, iv);
    if (m.nBF) caseSpeciesImplBoundaryFaceKernel<ST, W><<<gridOfS(m.nBF), QGD_BLOCK, 0, s>>>(m, c, g, sv, iv);
    implicitStatsMarkOn(S, stats, true);
    for (int a0 = 0, batch = 0; a0 < sv.nAct; a0 += W, ++batch) {
        const int nb = std::min(W, sv.nAct - a0);
        const int nr = nb == 1 ? 1 : (nb <= 3 ? 3 : 4);   // the solver's widths
        double gam[4] = {1.0, 1.0, 1.0, 1.0};
        for (int k = 0; k < nb; ++k) gam[k] = 1.0 / sv.Sc[sv.act[a0 + k]];
        caseSpeciesImplCellKernel<W><<<gridOfS(m.nC), QGD_BLOCK, 0, s>>>(m, c, sv, iv, a0, nr);
        implicitSolveSetup(S, nr, (1 << nb) - 1, iv.aF, iv.diag, iv.rhs, iv.x + (size_t)a0 * m.nC, tol, maxIter, gam);
        implicitSolveRun(S, nullptr);
        implicitSolveEndInto(S, stats, batch);
    }
    implicitStatsMarkOn(S, stats, false);
    if (sv.phiJmY && m.nF) caseSpeciesImplFluxKernel<W><<<gridOfS(m.nF), QGD_BLOCK, 0, s>>>(m, sv, iv);
    caseSpeciesImplClipKernel<W><<<gridOfS(m.nC), QGD_BLOCK, 0, s>>>(m, sv, iv);
    launchSpeciesPatchValues(s, m, sv);
}
void launchSpeciesAdvanceImplicit(hipStream_t s, int stencil, const MeshView& m, const CaseView& c, const GasModel& g, const SpeciesView& sv,
                                  const SpeciesImplView& iv, ImplicitSolver* S, double tol, int maxIter, double* stats) {
    if (m.nC == 0 || sv.nS == 0) return;
    switch (stencil) {
        case ST_REDUCED: launchSpeciesAdvanceImplicitT<ST_REDUCED>(s, m, c, g, sv, iv, S, tol, maxIter, stats); break;
        case ST_LSQ: launchSpeciesAdvanceImplicitT<ST_LSQ>(s, m, c, g, sv, iv, S, tol, maxIter, stats); break;
        case ST_GVP3: launchSpeciesAdvanceImplicitT<ST_GVP3>(s, m, c, g, sv, iv, S, tol, maxIter, stats); break;
        default: launchSpeciesAdvanceImplicitT<ST_GVP2>(s, m, c, g, sv, iv, S, tol, maxIter, stats); break;
    }
}

}  // namespace qgd
