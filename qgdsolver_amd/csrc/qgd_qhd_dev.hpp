// qgd_qhd_dev.hpp -- what the QHD step kernels (qgd_qhd.hip) and the QHD run monitor (qgd_qhd_monitor.hip) share: the compile-time modes
// of the step kernels and the body force of either solver.
#pragma once
#include <hip/hip_runtime.h>

#include "qgd_device.hpp"

namespace qgd {

// Compile-time modes of the step kernels (template parameter MODE).  MODE 0 is QHDFoam; the other instantiations are what
// qgd_qhd_case_set_srf / qgd_qhd_case_set_bc_values switch on: no uniform branch goes into the bodies.
//   QHD_ROT     SRFQHDFoam's body force (QhdBdFrc).  No centrifugal term, as in the listing: p is the reduced pressure.
//               gradWf = fvsc::grad(W) of updateFields.H L45 is not formed: nothing reads it.
//   QHD_FROZEN  no QHDTEqn.H in the loop [SRFQHDFoam.C L93-147]: T and T.boundary are not written
//   QHD_LIST    a fixedValue patch may carry one velocity per face (QhdView::bValU)
enum : int { QHD_ROT = 1, QHD_FROZEN = 2, QHD_LIST = 4 };

// BdFrc of one cell or patch face from its {Ux,Uy,Uz,T}: beta*T*g [updateFields.H L66], in the rotating frame beta*T*g - 2 (omega ^ U)
// with U the relative velocity [SRFQHDFoam/updateFields.H L73].  Per cell from the OLD U and T of that cell; on a patch face the same
// expression on the patch values U_b, T_b (BdFrc is a calculated field: qgdInterpolate takes its patch value).  The rotating form is
// evaluated where the object is made, all three components; the plain one component by component where [k] asks for it: the order in which
// the kernels always formed them (another order gives other registers and, in the rotating kernels, other FMA contractions)
template <int MODE>
struct QhdBdFrc {
    const QhdView& q;
    const double* u4;
    double B[3];
    static __device__ __forceinline__ void rot(const QhdView& q, const double* u4, double B[3]) {
        const double bT = q.beta * u4[3];
        B[0] = bT * q.g[0] - 2.0 * (q.omega[1] * u4[2] - q.omega[2] * u4[1]);
        B[1] = bT * q.g[1] - 2.0 * (q.omega[2] * u4[0] - q.omega[0] * u4[2]);
        B[2] = bT * q.g[2] - 2.0 * (q.omega[0] * u4[1] - q.omega[1] * u4[0]);
    }
    __device__ __forceinline__ QhdBdFrc(const QhdView& q_, const double* u4_) : q(q_), u4(u4_) {
        if (MODE & QHD_ROT) rot(q, u4, B);
    }
    __device__ __forceinline__ double operator[](const int k) const { return (MODE & QHD_ROT) ? B[k] : (q.beta * u4[3]) * q.g[k]; }
};

}  // namespace qgd
