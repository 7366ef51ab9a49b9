// qgd_species.hip -- the species block of reactingLagrangianQGDFoam resident in a QGDFoam case (gfx950 / CDNA4, wave64).
//
// A case with species (qgd_case_set_species) advances nS mass fractions Y_i with the flow, inside qgd_case_step, in the reference's
// order [reactingLagrangianQGDFoam_8C L92-140]: updateFluxes.H L103-132, QGDRhoEqn, QGDYEqn.H L38-92, QGDUEqn, QGDEEqn.  The composition
// is PASSIVE: every species shares the case's one `mixture` thermo; no chemistry (combustion->R), no parcel source, no feedback of Y into
// thermo.  This file: the explicit branch (QGDYEqn.H L67-86) and what both branches share; the implicitDiffusion branch (L47-66, the
// reference's default) is qgd_species_implicit.hip: the same vertex and face walks, then one linear solve per register batch.
//
//   SP  caseSpeciesPointKernel / caseSpeciesBoundaryPointKernel   GaussVolPoint: vertex values of ALL species in one walk over the points
//   SF  caseSpeciesFaceKernel<ST, W>        internal faces: labels, geometry, phiJm (plane 0 of CaseView::flux) and the two cells' records are
//                                       loaded once; tauQGDf, Uf, phi, muf are rebuilt from the records in registers (none of the four is
//                                       materialised); the species follow in register batches of W
//   SFB caseSpeciesBoundaryFaceKernel<ST, W> the same on patch faces (mirror-point stencil, patch records)
//   SC  caseSpeciesCellKernel<W>            one lane per cell over the cell -> face table, no atomics: rhoNew from phiJm and the device's deltaT
//                                       (the value the flow's cell update forms), then Y_i, Yi.max(0), Y_inert = max(1 - sum, 0)
//   SB  caseSpeciesPatchKernel              patch values for the next step
//   SH  caseSpeciesHaloKernel               the species tail of the state message (QGD_SPECIES_HALO): nS planes behind the flow's records
//
// SC and SB take the cell roles of cellUpdateKernel (mode / list): ghost cells and the patch faces of ghost cells are written by the unpack
// of the state message alone, a shard's boundary layer can go first.  SP, SF and SFB always walk everything: they read, and write only
// what SC reads.
//
// Per species the face kernels form [updateFluxes.H L122-127, QGDYEqn.H L75, L82]
//     gradYf, phiJmY_i = phiJm Yf_i - phi tauQGDf (Uf & gradYf), lap_i = (muf / Sc_i) snGrad(Y_i.old) |Sf|
// and write ONE number, phiJmY_i - lap_i, at the face's slot-major position (MeshView::fpos), so the cell kernel reads contiguously.
// With QGD_SPECIES_KEEP_FLUXES they also write phiJmY_i and diffusiveFlux_i by face label; the inert species' diffusiveFlux, cleared at
// updateFluxes.H L103-116, is minus the running sum of the others' [QGDYEqn.H L83].
//
// The gradients are those of qgd_stencil_dev.hpp (faceGradient: reduced, leastSquares 2-D, GaussVolPoint 2-D / 3-D with the nf*snGrad
// fallback on faces with more than four vertices and on degenerate faces), one call per species of a batch on the species' own plane:
// what does not depend on the species -- geometry loads, the GaussVolPoint coefficients -- is common to the calls of a batch.
#include "qgd_device.hpp"

#include "../../include/qgd_amd.h"
#include "qgd_species_dev.hpp"
#include "qgd_stencil_dev.hpp"

namespace qgd {

template <int ST, int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesFaceKernel(const MeshView m, const CaseView c, const GasModel gm, const SpeciesView sv) {
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
    double inertDf = 0.0;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) speciesBatch<ST, W, true, false>(m, sv, F, f, pos, a0, inertDf);
    if (sv.phiJmY) {
        sv.phiJmY[(size_t)sv.inert * m.nF + f] = 0.0;
        sv.dflux[(size_t)sv.inert * m.nF + f] = inertDf;
    }
}

template <int ST, int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesBoundaryFaceKernel(const MeshView m, const CaseView c, const GasModel gm, const SpeciesView sv) {
    const int b = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (b >= m.nBF) return;
    const int f = m.nIF + b;
    const size_t nF = (size_t)m.nF;
    if (m.fkind[f] == 3) {   // empty patches carry no field
        for (int a = 0; a < sv.nAct; ++a) sv.F[(size_t)a * nF + f] = 0.0;
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
    double inertDf = 0.0;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) speciesBatch<ST, W, false, false>(m, sv, F, f, (size_t)f, a0, inertDf);
    if (sv.phiJmY) {
        sv.phiJmY[(size_t)sv.inert * nF + f] = 0.0;
        sv.dflux[(size_t)sv.inert * nF + f] = inertDf;
    }
}

// vertex values of every species: the weights of launchPointInterp (volPointInterpolation's, pointCells order), read once per batch
template <int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesPointKernel(const MeshView m, const SpeciesView sv) {
    const int p = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (p >= m.nP) return;
    const int n = m.pcCount[p];
    if (n == 0) return;   // patch point: caseSpeciesBoundaryPointKernel
    const size_t base = (size_t)m.pcSlice[p >> 6] * 64 + (p & 63);
    const size_t nC = (size_t)m.nC, nP = (size_t)m.nP;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) {
        int sp[W];
        double acc[W];
#pragma unroll
        for (int k = 0; k < W; ++k) { sp[k] = sv.act[min(a0 + k, sv.nAct - 1)]; acc[k] = 0.0; }
        for (int i = 0; i < n; ++i) {
            const double w = m.pcW[base + (size_t)i * 64];
            const size_t cell = (size_t)m.pcCell[base + (size_t)i * 64];
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] += w * sv.Y[(size_t)sp[k] * nC + cell];
        }
#pragma unroll
        for (int k = 0; k < W; ++k) if (a0 + k < sv.nAct) sv.ptY[(size_t)(a0 + k) * nP + p] = acc[k];
    }
}
// patch points: the weights of launchBoundaryPoints (scalars: no point constraints apply)
template <int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesBoundaryPointKernel(const MeshView m, const SpeciesView sv) {
    const int i = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (i >= m.nBP) return;
    const int p = m.bpPoint[i];
    const int e0 = m.bpOff[i], e1 = m.bpOff[i + 1];
    const size_t nBF = (size_t)m.nBF, nP = (size_t)m.nP;
    for (int a0 = 0; a0 < sv.nAct; a0 += W) {
        int sp[W];
        double acc[W];
#pragma unroll
        for (int k = 0; k < W; ++k) { sp[k] = sv.act[min(a0 + k, sv.nAct - 1)]; acc[k] = 0.0; }
        for (int e = e0; e < e1; ++e) {
            const double w = m.bpW[e];
            const size_t bf = (size_t)m.bpFace[e];
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] += w * sv.Yb[(size_t)sp[k] * nBF + bf];
        }
#pragma unroll
        for (int k = 0; k < W; ++k) if (a0 + k < sv.nAct) sv.ptY[(size_t)(a0 + k) * nP + p] = acc[k];
    }
}

// QGDYEqn.H L67-91 of one cell: fvm::ddt(rho, Yi) + fvc::div(phiJmYi - lap_i) == 0 (Euler), the divergence gathered in ascending face
// label like fvc::surfaceIntegrate; rho.oldTime() is the record's density (the flow's cell update runs after this kernel), rho the value
// that update forms from the same mass fluxes and the same deltaT [QGDRhoEqn_8H L40-47]
// mode 0: every cell but the ghosts; mode 1: the cells of `list` (a shard's boundary layer); mode 2: ordinary owned cells only -- the
// convention of cellUpdateKernel.  Without cell roles (MeshView::ghost null) mode 0 is every cell.
template <int W>
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesCellKernel(const MeshView m, const CaseView c, const SpeciesView sv, const int mode,
                                                                  const int32_t* __restrict__ list, const int nList) {
    const int idx = blockIdx.x * QGD_BLOCK + threadIdx.x;
    int ci;
    if (mode == 1) { if (idx >= nList) return; ci = list[idx]; }
    else {
        if (idx >= m.nC) return;
        const int role = m.ghost ? m.ghost[idx] : 0;
        if (role == 1 || (mode == 2 && role == 2)) return;
        ci = idx;
    }
    const int n = m.cfCount[ci];
    const size_t base = (size_t)m.cfSlice[ci >> 6] * 64 + (ci & 63);
    const size_t nC = (size_t)m.nC, nF = (size_t)m.nF;
    double sum0 = 0.0;
    for (int i = 0; i < n; ++i) {
        const int it = m.cfPos[base + (size_t)i * 64];
        const double x = c.flux[(size_t)(it >= 0 ? it : ~it)];
        sum0 = it >= 0 ? sum0 + x : sum0 - x;
    }
    const double V = m.V[ci], dt = c.dt[0];
    const double rhoOld = c.A[ci].rho;
    const double dtV = dt / V;
    const double rhoNew = rhoOld - dtV * sum0;
    const double rDeltaT = 1.0 / dt;
    const double den = rDeltaT * rhoNew * V;
    double Yt = 0.0;                                                   // volScalarField Yt(0.0*Y[0]) [L38]
    for (int a0 = 0; a0 < sv.nAct; a0 += W) {
        int sp[W];
        double s[W];
#pragma unroll
        for (int k = 0; k < W; ++k) { sp[k] = sv.act[min(a0 + k, sv.nAct - 1)]; s[k] = 0.0; }
        for (int i = 0; i < n; ++i) {
            const int it = m.cfPos[base + (size_t)i * 64];
            const size_t pos = (size_t)(it >= 0 ? it : ~it);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const double x = sv.F[(size_t)min(a0 + k, sv.nAct - 1) * nF + pos];
                s[k] = it >= 0 ? s[k] + x : s[k] - x;
            }
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (a0 + k < sv.nAct) {
                double* __restrict__ y = sv.Y + (size_t)sp[k] * nC + ci;
                const double yn = fmax((rDeltaT * rhoOld * (*y) * V - s[k]) / den, 0.0);   // solve(...) [L69-80]; Yi.max(0.0) [L86]
                *y = yn;
                Yt += yn;                                                                  // [L87]
            }
        }
    }
    sv.Y[(size_t)sv.inert * nC + ci] = fmax(1.0 - Yt, 0.0);                                // [L90-91]
}

// patch values of every species: fixedValue keeps its value, zeroGradient (and the constraint patches' `none`) takes the owner's.
// Modes as in caseSpeciesCellKernel, by the role of the face's owner cell (mode 1: the patch faces of `list`, which the unpack of the state
// message uses for the patch faces of a slot's ghost cells too); mode < 0 evaluates every face (the first evaluation, from the caller's fields)
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesPatchKernel(const MeshView m, const SpeciesView sv, const int mode,
                                                                   const int32_t* __restrict__ list, const int nList) {
    const int idx = blockIdx.x * QGD_BLOCK + threadIdx.x;
    int b;
    if (mode == 1) { if (idx >= nList) return; b = list[idx]; }
    else { if (idx >= m.nBF) return; b = idx; }
    const int o = m.own[m.nIF + b], patch = m.bPatch[b];
    if (mode != 1 && mode >= 0 && m.ghost) {
        const int role = m.ghost[o];
        if (role == 1 || (mode == 2 && role == 2)) return;
    }
    for (int i = 0; i < sv.nS; ++i) {
        const size_t e = (size_t)i * sv.nPatches + patch;
        sv.Yb[(size_t)i * m.nBF + b] = sv.bcKind[e] == QGD_BC_FIXEDVALUE ? sv.bcVal[e] : sv.Y[(size_t)i * m.nC + o];
    }
}

// The species tail of the state message: nS planes of n doubles behind the flow's records, species-major, so that a wavefront's stores on
// pack and loads on unpack are contiguous; one lane per entry of the slot's cell list (send cells on pack, ghost cells on unpack), all nS
// species -- the inert one too: a ghost cell holds its original's whole composition.  Patch values do not travel: the unpack re-evaluates
// those of the slot's ghost patch faces from the patch rule (caseSpeciesPatchKernel on that list), as the state message does c and alpha/c.
__global__ __launch_bounds__(QGD_BLOCK) void caseSpeciesHaloKernel(const SpeciesView sv, const int nC, const int32_t* __restrict__ cells, const int n,
                                                                  double* __restrict__ tail, const int pack) {
    const int i = blockIdx.x * QGD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t ci = (size_t)cells[i];
    if (pack) for (int s = 0; s < sv.nS; ++s) tail[(size_t)s * n + i] = sv.Y[(size_t)s * nC + ci];
    else for (int s = 0; s < sv.nS; ++s) sv.Y[(size_t)s * nC + ci] = tail[(size_t)s * n + i];
}

void launchSpeciesPatchValues(hipStream_t s, const MeshView& m, const SpeciesView& sv, int mode, const int32_t* list, int nList) {
    const int n = (mode == 1) ? nList : m.nBF;
    if (n) caseSpeciesPatchKernel<<<gridOfS(n), QGD_BLOCK, 0, s>>>(m, sv, mode, list, nList);
}
void launchSpeciesHalo(hipStream_t s, const MeshView& m, const SpeciesView& sv, const int32_t* cells, int32_t nCells, const int32_t* bfaces,
                       int32_t nFaces, double* tail, bool pack) {
    if (nCells) caseSpeciesHaloKernel<<<gridOfS(nCells), QGD_BLOCK, 0, s>>>(sv, m.nC, cells, nCells, tail, pack ? 1 : 0);
    if (!pack) launchSpeciesPatchValues(s, m, sv, 1, bfaces, nFaces);   // behind the cells on the same stream: the faces' owners are among them
}

// vertex values of the transported species (GaussVolPoint): the implicit branch's walk (qgd_species_implicit.hip) starts with them too
void launchSpeciesPoints(hipStream_t s, const MeshView& m, const SpeciesView& sv) {
    constexpr int W = QGD_SPECIES_W;
    caseSpeciesPointKernel<W><<<gridOfS(m.nP), QGD_BLOCK, 0, s>>>(m, sv);
    if (m.nBP) caseSpeciesBoundaryPointKernel<W><<<gridOfS(m.nBP), QGD_BLOCK, 0, s>>>(m, sv);
}

// part 0: everything; part 1: the walks over ALL faces, then the cells of `list` and the patch faces of `blist` (a shard's boundary layer);
// part 2: the remaining owned cells and their patch faces, from the face values part 1 left
template <int ST>
static void launchSpeciesAdvanceT(hipStream_t s, const MeshView& m, const CaseView& c, const GasModel& g, const SpeciesView& sv, int part,
                                  const int32_t* list, int nList, const int32_t* blist, int nBList) {
    constexpr int W = QGD_SPECIES_W;
    if (part != 2) {
        if (ST == ST_GVP3 || ST == ST_GVP2) launchSpeciesPoints(s, m, sv);
        if (m.nIF) caseSpeciesFaceKernel<ST, W><<<gridOfS(m.nIF), QGD_BLOCK, 0, s>>>(m, c, g, sv);
        if (m.nBF) caseSpeciesBoundaryFaceKernel<ST, W><<<gridOfS(m.nBF), QGD_BLOCK, 0, s>>>(m, c, g, sv);
    }
    const int n = (part == 1) ? nList : m.nC;
    if (n) caseSpeciesCellKernel<W><<<gridOfS(n), QGD_BLOCK, 0, s>>>(m, c, sv, part, list, nList);
    launchSpeciesPatchValues(s, m, sv, part, blist, nBList);
}
void launchSpeciesAdvance(hipStream_t s, int stencil, const MeshView& m, const CaseView& c, const GasModel& g, const SpeciesView& sv, int part,
                          const int32_t* list, int nList, const int32_t* blist, int nBList) {
    if (m.nC == 0 || sv.nS == 0) return;
    switch (stencil) {
        case ST_REDUCED: launchSpeciesAdvanceT<ST_REDUCED>(s, m, c, g, sv, part, list, nList, blist, nBList); break;
        case ST_LSQ: launchSpeciesAdvanceT<ST_LSQ>(s, m, c, g, sv, part, list, nList, blist, nBList); break;
        case ST_GVP3: launchSpeciesAdvanceT<ST_GVP3>(s, m, c, g, sv, part, list, nList, blist, nBList); break;
        default: launchSpeciesAdvanceT<ST_GVP2>(s, m, c, g, sv, part, list, nList, blist, nBList); break;
    }
}
int speciesBatchWidth() { return QGD_SPECIES_W; }

}  // namespace qgd
