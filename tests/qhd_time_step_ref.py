"""Reference of the time-step control of QHDFoam / SRFQHDFoam [QHDCourantNo.H L37-57, setDeltaT-QGDQHD.H L41-61] in numpy, from the mesh
and the CPU oracle's fluxes: nothing here reads a quantity the device reduced."""
import numpy as np

from qgdsolver_amd import _lib as L

import oracle
from scalar_ref import delta_t_rule


def h_qgd_f(mesh):
    """(hQGDf, live): QGDCoeffs::updateQGDLength restated [QGDCoeffs.C L195-199, L303-317] -- 2 min(|C_O - Cf|, |C_N - Cf|) on internal faces,
    2 / |deltaCoeffs| on patch faces; live marks the faces that carry a field (not those of empty patches), hQGDf is 0 elsewhere"""
    nif, nF = mesh.nInternalFaces, mesh.nFaces
    C, Cf = mesh.array("C").reshape(-1, 3), mesh.array("Cf").reshape(-1, 3)
    own, nei = mesh.array("owner"), mesh.array("neighbour")
    h = np.zeros(nF)
    h[:nif] = 2.0 * np.minimum(np.linalg.norm(C[own[:nif]] - Cf[:nif], axis=1), np.linalg.norm(C[nei[:nif]] - Cf[:nif], axis=1))
    h[nif:] = 2.0 * (1.0 / np.abs(mesh.array("deltaCoeffs")[nif:]))
    live = np.ones(nF, dtype=bool)
    for st, n, t in zip(mesh.array("patchStart"), mesh.array("patchSize"), mesh.array("patchType")):
        if t == L.PATCH_EMPTY:
            live[int(st): int(st) + int(n)] = False
    h[~live] = 0.0
    return h, live


class CourantRef:
    """max |Unf| / hQGDf of a state [QHDCourantNo.H L44-48]: phiu = Sf & Uf from the oracle's qhd_fluxes on the state's cell and patch
    values, |Sf| from the mesh, hQGDf restated from the mesh"""

    def __init__(self, mesh, omesh, stencil, rho0, tau_f):
        self.mesh, self.om, self.stencil = mesh, omesh, stencil
        self.h, self.live = h_qgd_f(mesh)
        self.magSf = mesh.array("magSf")
        self.rho = (np.full(mesh.nCells, rho0), np.full(mesh.nBoundaryFaces, rho0))
        self.tau = np.asarray(tau_f)
        self.min_tau = float(self.tau[self.live].min())

    def per_face(self, U, Ub, T, Tb):
        phiu = oracle.qhd_fluxes(self.om, self.stencil, (U, Ub), (T, Tb), self.rho, self.tau, 0.0, (0.0, 0.0, 0.0))["phiu"]
        cof = np.zeros(self.mesh.nFaces)
        cof[self.live] = np.abs(phiu[self.live]) / self.magSf[self.live] / self.h[self.live]
        return cof

    def max_unf_by_h(self, case):
        return float(self.per_face(case.field("U"), case.field("U.boundary"), case.field("T"), case.field("T.boundary")).max())

    def rule(self, dt, max_ubyh, max_co, max_delta_t, c_tau):
        """(CoNum the control sees, the new deltaT)"""
        return delta_t_rule(dt, max_ubyh, self.min_tau, max_co, max_delta_t, c_tau)
