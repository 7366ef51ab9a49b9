// qgd_species_dev.hpp -- what the face walks of the species block share (qgd_species.hip: the explicit branch; qgd_species_implicit.hip: the
// implicitDiffusion branch): the register batch, what a face knows before the species come, the species of a batch on one face.
#pragma once
#include "qgd_device.hpp"
#include "qgd_stencil_dev.hpp"

namespace qgd {

#define QGD_SPECIES_W 4   // species per register batch (qgd_case_species_info reports it; profiles/kernel_resources.txt lists the instantiations: none spills)

static inline int gridOfS(int64_t n) { return (int)((n + QGD_BLOCK - 1) / QGD_BLOCK); }

// what a face knows before the species come: loaded / rebuilt once
struct SpeciesFace {
    double phiJm, phiTau, Uf[3], mufS;   // phiTau = phi tauQGDf; mufS = muf |Sf|
    double w, dn;
    int o, n;                            // n: neighbour cell (internal) or boundary face index (patch)
};

// the species a0 .. a0 + W - 1 of the transported ones on one face (slots past the last species repeat it and store nothing)
template <int ST, int W, bool INTERNAL, bool IMPL>
__device__ __forceinline__ void speciesBatch(const MeshView& m, const SpeciesView& sv, const SpeciesFace& F, const int f, const size_t pos,
                                             const int a0, double& inertDf) {
    const size_t nC = (size_t)m.nC, nP = (size_t)m.nP, nF = (size_t)m.nF, nBF = (size_t)m.nBF;
    int sp[W], slot[W];   // the species' label, and its place among the transported ones: the planes of F and ptY
    FaceVals<1> v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        slot[k] = min(a0 + k, sv.nAct - 1);
        sp[k] = sv.act[slot[k]];
        const double* __restrict__ Y = sv.Y + (size_t)sp[k] * nC;
        v[k].o[0] = Y[F.o];
        if (INTERNAL) { v[k].n[0] = Y[F.n]; v[k].sn[0] = 0.0; }
        else { v[k].n[0] = sv.Yb[(size_t)sp[k] * nBF + F.n]; v[k].sn[0] = F.dn * (v[k].n[0] - v[k].o[0]); }   // fvPatchField::snGrad (L0)
    }
    double g[W][3];
#pragma unroll
    for (int k = 0; k < W; ++k)
        faceGradient<ST, 1, -1>(m, f, v[k], sv.Y + (size_t)sp[k] * nC, sv.ptY ? sv.ptY + (size_t)slot[k] * nP : nullptr, g[k]);
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const double Yf = INTERNAL ? lerpf(F.w, v[k].o[0], v[k].n[0]) : v[k].n[0];
        const double dydt = (-F.phiTau) * (F.Uf[0] * g[k][0] + F.Uf[1] * g[k][1] + F.Uf[2] * g[k][2]);   // [updateFluxes.H L124-125]
        const double pjy = F.phiJm * Yf + dydt;                                                          // [L123, L126]
        const double sn = INTERNAL ? F.dn * (v[k].n[0] - v[k].o[0]) : v[k].sn[0];
        const double lap = IMPL ? 0.0 : (F.mufS / sv.Sc[sp[k]]) * sn;                                    // [QGDYEqn.H L75, L82]; IMPL: the laplacian is the solve's
        if (a0 + k < sv.nAct) {
            sv.F[(size_t)slot[k] * nF + pos] = pjy - lap;
            if (sv.phiJmY) {
                const double df = dydt + lap;
                sv.phiJmY[(size_t)sp[k] * nF + f] = pjy;
                sv.dflux[(size_t)sp[k] * nF + f] = df;
                inertDf -= df;                                                                            // [QGDYEqn.H L83]
            }
        }
    }
}

}  // namespace qgd
