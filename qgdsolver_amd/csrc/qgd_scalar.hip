// qgd_scalar.hip -- scalarTransportQHDFoam resident on the device (scalarTransportQHDFoam_8C_source.html L86-125, with its createFields.H,
// createFaceFields.H, createFaceFluxes.H, updateFluxes.H, updateFields.H):
//
//   once      thermo.correct(): rho, alpha, tauQGDf, hQGDf fixed; Uf = qgdInterpolate(U), phiu = Sf & Uf [updateFluxes.H L3-4]
//   per step  gradTf = fvsc::grad(T), Tf = qgdInterpolate(T), Hif = alphaf/rhof [updateFields.H L1-9]
//             phiTf = qgdFlux(phiu,T,Tf), phiTauTReg = tauQGDf phiu (Uf & gradTf) [.C L110-111]
//             solve(fvm::ddt(T) + fvc::div(phiTf) - fvc::Sp(fvc::div(phiu),T) - fvm::laplacian(Hif,T) - fvc::div(phiTauTReg) == TSu) [.C L115-123]
//
// U is read and never advanced, the thermo is rhoConst + constTransport (uniform rho0, mu, Pr; the QHD closures leave alphauQGD = 0, so
// Hif = mu/(Pr rho0)): everything that does not depend on T -- phiu, tauQGDf phiu Uf, the matrix coefficients a_f = Hif |Sf| delta_f, the
// volume-integrated div(phiu), the patch sources a_b T_b of fixedValue faces -- is formed ONCE (scalarSetup*Kernel).  A step is then
//   patch values of T | vertex values of T (GaussVolPoint) | one face kernel: F_f = phiu Tf - (tau phiu Uf) & gradTf | one cell kernel:
//   rhs_P = V/deltaT T_P - sum +-F_f + divPhiu_P T_P + sum a_b T_b | the solve (qgd_implicit.hip, one right-hand side, T itself is the
//   iterate: the start value is the old T and the solution needs no copy).
// L0 discretisation as in qgd_qhd.hip: Euler ddt, fvc::div = surfaceIntegrate in ascending face label, Gauss linear uncorrected laplacian.
#include <algorithm>

#include "../../include/qgd_amd.h"
#include "qgd_device.hpp"
#include "qgd_stencil_dev.hpp"

namespace qgd {

namespace {

inline int gridOf(int64_t n) { return (int)((n + QGD_BLOCK - 1) / QGD_BLOCK); }

// tauQGD of the QHD closures [constTau_8C L71-74, HbyUQHD_8C L80-83, T0byGr_8C L84-87, H2bynuQHD_8C L78-82]
__device__ __forceinline__ double scalarTauOf(const ScalarView& q, const double h) {
    switch (q.tauModel) {
        case 0: return q.Tau;
        case 1: return q.aQGD * h / q.UQHD;
        case 2: return q.T0 / q.Gr;
        default: return q.aQGD * h * h / q.nu;
    }
}

// ---- set-up ----------------------------------------------------------------------------------------------------------------------------
// per face: tauQGDf = linearInterpolate(tauQGD), Uf (patch faces: U's boundary condition evaluated on the owner's velocity), phiu,
// tauQGDf phiu Uf, a_f at the face's slot-major position; per workgroup max |Uf|/hQGDf and min tauQGDf over the non-empty faces
__global__ __launch_bounds__(QGD_BLOCK) void scalarSetupFaceKernel(const MeshView m, const ScalarView q, const PatchBCDev* __restrict__ bcs,
                                                                  const double* __restrict__ U, double* __restrict__ part) {
    const int f = blockIdx.x * QGD_BLOCK + threadIdx.x;
    double co = -1e300, mt = 1e300;
    if (f < m.nF) {
        const size_t nF = (size_t)m.nF, pos = f < m.nIF ? (size_t)m.fpos[f] : (size_t)f;
        double uf[3] = {0, 0, 0}, tau = 0.0, phiu = 0.0, a = 0.0;
        if (m.fkind[f] != 3) {
            const int o = m.own[f];
            const double uo[3] = {U[3 * (size_t)o], U[3 * (size_t)o + 1], U[3 * (size_t)o + 2]};
            if (f < m.nIF) {
                const int n = m.nei[f];
                const double w = m.w[f];
#pragma unroll
                for (int k = 0; k < 3; ++k) uf[k] = lerpf(w, uo[k], U[3 * (size_t)n + k]);
                tau = lerpf(w, scalarTauOf(q, m.hQGD[o]), scalarTauOf(q, m.hQGD[n]));
            } else {
                const int b = f - m.nIF;
                const PatchBCDev bc = bcs[m.bPatch[b]];
                // (vU / vT throughout this file: the scalar case has one value per patch and entry; per-face lists, PatchBCDev::valList,
                // belong to the QGDFoam case)
                if (bc.bcU == QGD_BC_FIXEDVALUE) { uf[0] = bc.vU[0]; uf[1] = bc.vU[1]; uf[2] = bc.vU[2]; }
                else if (bc.bcU == QGD_BC_SLIP) {   // basicSymmetry::evaluate = (pif + transform(I - 2 nn, pif))/2
                    double n[3];
                    symmNormal(m, bc, f, n);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double tv = ((i == 0 ? 1.0 : 0.0) - 2.0 * (n[i] * n[0])) * uo[0] + ((i == 1 ? 1.0 : 0.0) - 2.0 * (n[i] * n[1])) * uo[1] +
                                          ((i == 2 ? 1.0 : 0.0) - 2.0 * (n[i] * n[2])) * uo[2];
                        uf[i] = (uo[i] + tv) / 2.0;
                    }
                } else { uf[0] = uo[0]; uf[1] = uo[1]; uf[2] = uo[2]; }
                tau = scalarTauOf(q, m.hQGDb[b]);
            }
            phiu = m.Sx[f] * uf[0] + m.Sy[f] * uf[1] + m.Sz[f] * uf[2];
            a = q.Hi * m.magSf[f] * m.dn[f];   // nonOrthDeltaCoeffs inside, deltaCoeffs on patches
            co = sqrt(uf[0] * uf[0] + uf[1] * uf[1] + uf[2] * uf[2]) / m.hf[f];
            mt = tau;
        }
        q.tauF[f] = tau;
        q.phiu[f] = phiu;
        const double tp = tau * phiu;
#pragma unroll
        for (int k = 0; k < 3; ++k) { q.Uf[(size_t)k * nF + f] = uf[k]; q.tpu[(size_t)k * nF + f] = tp * uf[k]; }
        q.a[pos] = a;
    }
    blockMaxMin(co, mt, part + 2 * (size_t)blockIdx.x, false);
}
// second level of the reduction: one workgroup folds the partials into red = {max |Uf|/hQGDf, min tauQGDf}
__global__ __launch_bounds__(QGD_BLOCK) void scalarSetupFoldKernel(const double* __restrict__ part, const int n, double* __restrict__ red) {
    double co = -1e300, mt = 1e300;
    for (int i = threadIdx.x; i < n; i += QGD_BLOCK) { co = fmax(co, part[2 * (size_t)i]); mt = fmin(mt, part[2 * (size_t)i + 1]); }
    blockMaxMin(co, mt, red, false);
}
// per cell: T, the volume-integrated div(phiu) (surfaceIntegrate without the division by V: the equation multiplies it back), the sum of the
// matrix coefficients of the cell's internal and fixedValue patch faces, the patch sources a_b T_b
__global__ __launch_bounds__(QGD_BLOCK) void scalarSetupCellKernel(const MeshView m, const ScalarView q, const PatchBCDev* __restrict__ bcs,
                                                                  const double* __restrict__ T) {
    const int c = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (c >= m.nC) return;
    const int n = m.cfCount[c];
    const size_t base = (size_t)m.cfSlice[c >> 6] * 64 + (c & 63);
    double dv = 0.0, ds = 0.0, sb = 0.0;
    for (int i = 0; i < n; ++i) {
        const int it = m.cfItem[base + (size_t)i * 64], ps = m.cfPos[base + (size_t)i * 64];
        const int f = it >= 0 ? it : ~it;
        if (m.fkind[f] == 3) continue;
        const double ph = q.phiu[f];
        dv = it >= 0 ? dv + ph : dv - ph;
        const double af = q.a[ps >= 0 ? ps : ~ps];
        if (f < m.nIF) { ds += af; continue; }
        const PatchBCDev bc = bcs[m.bPatch[f - m.nIF]];
        if (bc.bcT == QGD_BC_FIXEDVALUE) { ds += af; sb += af * bc.vT; }   // zeroGradient: nothing
    }
    q.T[c] = T[c];
    q.divPhiu[c] = dv;
    q.diagBase[c] = ds;
    q.srcB[c] = sb;
}
__global__ __launch_bounds__(QGD_BLOCK) void scalarDiagKernel(const MeshView m, const ScalarView q, const double rDeltaT) {
    const int c = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (c < m.nC) q.diag[c] = rDeltaT * m.V[c] + q.diagBase[c];
}

// ---- per step --------------------------------------------------------------------------------------------------------------------------
// T.correctBoundaryConditions(): fixedValue | zeroGradient (constraint patches: zero-gradient scalars)
__global__ __launch_bounds__(QGD_BLOCK) void scalarBcKernel(const MeshView m, const ScalarView q, const PatchBCDev* __restrict__ bcs) {
    const int b = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (b >= m.nBF) return;
    const int f = m.nIF + b;
    const int o = m.own[f];
    const int pi = m.bPatch[b];
    const double To = q.T[o];
    const PatchBCDev bc = bcs[pi];
    q.Tb[b] = bc.bcT == QGD_BC_FIXEDVALUE ? bc.vT : To;
}

// the face kernel [updateFields.H L1-9, .C L110-111]: gradTf by the stencil's shared gradient function, Tf linear or upwind, the net face
// flux F_f = phiu Tf - (tau phiu Uf) & gradTf at the face's slot-major position.  DBG: the three listed fields into q.dbg instead.
template <int ST, bool DBG>
__global__ __launch_bounds__(QGD_BLOCK) void scalarFaceKernel(const MeshView m, const ScalarView q, const PatchBCDev* __restrict__ bcs) {
    const int f = xcdTile((int)gridDim.x, m.xcdRun) * QGD_BLOCK + (int)threadIdx.x;   // runs of consecutive blocks per XCD: neighbours meet in one L2
    if (f >= m.nF) return;
    const size_t nF = (size_t)m.nF;
    const bool internal = f < m.nIF;
    // everything whose address is known from f alone is asked for before the first label is used
    const int o = m.own[f];
    const int nOrB = internal ? m.nei[f] : f - m.nIF;
    const int kind = m.fkind[f];
    const size_t pos = internal ? (size_t)m.fpos[f] : (size_t)f;
    const double w = m.w[f], phiu = q.phiu[f];
    const double tp[3] = {q.tpu[f], q.tpu[nF + f], q.tpu[2 * nF + f]};
    FaceVals<1> v;
    v.o[0] = q.T[o];
    v.sn[0] = 0.0;
    if (internal) v.n[0] = q.T[nOrB];
    else {
        v.n[0] = q.Tb[nOrB];
        // fvPatchField::snGrad = deltaCoeffs (value - internal) on fixedValue patches, zero on zeroGradient ones
        if (kind != 3 && bcs[m.bPatch[nOrB]].bcT == QGD_BC_FIXEDVALUE) v.sn[0] = m.dn[f] * (v.n[0] - v.o[0]);
    }
    if (kind == 3) {
        if (DBG) { for (int k = 0; k < 5; ++k) q.dbg[(size_t)k * nF + f] = 0.0; }
        else q.F[pos] = 0.0;
        return;
    }
    double g[3];
    faceGradient<ST, 1, -1>(m, f, v, q.T, q.ptT, g);
    // qgdFlux(phiu,T,Tf) [QGDInterpolate.H L86-104]: phiu Tf, or with `div(phiu,T) Gauss upwind` phiu (pos0(phiu) (T_O - T_N) + T_N) inside,
    // the patch value on patch faces
    const double Tf = internal ? ((q.upwindT) ? lerpf(phiu >= 0.0 ? 1.0 : 0.0, v.o[0], v.n[0]) : lerpf(w, v.o[0], v.n[0])) : v.n[0];
    const double phiTf = phiu * Tf;
    const double reg = tp[0] * g[0] + tp[1] * g[1] + tp[2] * g[2];   // tauQGDf phiu (Uf & gradTf)
    if (DBG) {
        q.dbg[0 * nF + f] = g[0]; q.dbg[1 * nF + f] = g[1]; q.dbg[2 * nF + f] = g[2];
        q.dbg[3 * nF + f] = phiTf; q.dbg[4 * nF + f] = reg;
    } else q.F[pos] = phiTf - reg;
}

// the cell kernel [.C L115-123]: the ordered sum of the net face fluxes through their slot-major positions (ascending face label: cfPos keeps
// cfItem's order), rhs_P = V/deltaT T_P - sum +-F_f + divPhiu_P T_P + sum a_b T_b
__global__ __launch_bounds__(QGD_BLOCK) void scalarRhsKernel(const MeshView m, const ScalarView q, const double rDeltaT) {
    const int c = xcdTile((int)gridDim.x, m.xcdRun) * QGD_BLOCK + threadIdx.x;
    if (c >= m.nC) return;
    const int n = m.cfCount[c];
    const size_t base = (size_t)m.cfSlice[c >> 6] * 64 + (c & 63);
    const double T = q.T[c], V = m.V[c], dv = q.divPhiu[c], sb = q.srcB[c];
    double s = 0.0;
    if (__ballot(n != 6) == 0) {
        // a wavefront of hexahedra: the six positions, then the six terms in flight before the ordered sum
        int it[6];
        double x[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) it[i] = m.cfPos[base + (size_t)i * 64];
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] = q.F[(size_t)(it[i] >= 0 ? it[i] : ~it[i])];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 6; ++i) s = it[i] >= 0 ? s + x[i] : s - x[i];
    } else {
        for (int i0 = 0; i0 < n; i0 += 8) {   // any cell shapes: eight faces per pass
            int it[8];
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) it[u] = i0 + u < n ? m.cfPos[base + (size_t)(i0 + u) * 64] : 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = i0 + u < n ? q.F[(size_t)(it[u] >= 0 ? it[u] : ~it[u])] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u >= n) continue;
                s = it[u] >= 0 ? s + x[u] : s - x[u];
            }
        }
    }
    q.rhs[c] = ((rDeltaT * T * V - s) + dv * T) + sb;
}

template <int ST>
void faces(hipStream_t s, const MeshView& m, const ScalarView& q, const PatchBCDev* bc, bool dbg) {
    if (m.nF == 0) return;
    if (dbg) scalarFaceKernel<ST, true><<<gridOf(m.nF), QGD_BLOCK, 0, s>>>(m, q, bc);
    else scalarFaceKernel<ST, false><<<gridOf(m.nF), QGD_BLOCK, 0, s>>>(m, q, bc);
}

}  // namespace

void launchScalarSetup(hipStream_t s, const MeshView& m, const ScalarView& q, const PatchBCDev* bc, const double* U, const double* T, double* work,
                       double* red) {
    const int gf = gridOf(std::max(m.nF, 1));
    scalarSetupFaceKernel<<<gf, QGD_BLOCK, 0, s>>>(m, q, bc, U, work);
    scalarSetupFoldKernel<<<1, QGD_BLOCK, 0, s>>>(work, gf, red);
    scalarSetupCellKernel<<<gridOf(m.nC), QGD_BLOCK, 0, s>>>(m, q, bc, T);
    if (m.nBF) scalarBcKernel<<<gridOf(m.nBF), QGD_BLOCK, 0, s>>>(m, q, bc);
}
void launchScalarDiag(hipStream_t s, const MeshView& m, const ScalarView& q, double dt) {
    scalarDiagKernel<<<gridOf(m.nC), QGD_BLOCK, 0, s>>>(m, q, 1.0 / dt);
}
void launchScalarPatchValues(hipStream_t s, const MeshView& m, const ScalarView& q, const PatchBCDev* bc) {
    if (m.nBF) scalarBcKernel<<<gridOf(m.nBF), QGD_BLOCK, 0, s>>>(m, q, bc);
}
void launchScalarAssemble(hipStream_t s, int stencil, bool usesPoints, const MeshView& m, const ScalarView& q, const PatchBCDev* bc, double dt,
                          bool rhs) {
    if (m.nBF) scalarBcKernel<<<gridOf(m.nBF), QGD_BLOCK, 0, s>>>(m, q, bc);
    if (usesPoints) {   // the vertex values of T: the scheme of every GaussVolPoint path here (volPointInterpolation; patch points from the patch values)
        pointInterpFastKernel<1><<<gridOf(m.nP), QGD_BLOCK, 0, s>>>(m, q.T, q.ptT);
        if (m.nBP) boundaryPointKernel<1><<<gridOf(m.nBP), QGD_BLOCK, 0, s>>>(m, q.Tb, 1, q.ptT, 1, 0, -1);
    }
    const bool dbg = !rhs;
    switch (stencil) {
        case ST_REDUCED: faces<ST_REDUCED>(s, m, q, bc, dbg); break;
        case ST_LSQ: faces<ST_LSQ>(s, m, q, bc, dbg); break;
        case ST_GVP3: faces<ST_GVP3>(s, m, q, bc, dbg); break;
        default: faces<ST_GVP2>(s, m, q, bc, dbg); break;
    }
    if (rhs) scalarRhsKernel<<<gridOf(m.nC), QGD_BLOCK, 0, s>>>(m, q, 1.0 / dt);
}

}  // namespace qgd
