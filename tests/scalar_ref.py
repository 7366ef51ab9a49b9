"""The step of scalarTransportQHDFoam [scalarTransportQHDFoam.C L86-125] restated in numpy for ANY mesh: the yardstick of the resident
device case (qgdsolver_amd.scalarfoam), independent of it.

  phiu, gradTf, phiTauTReg    oracle.qhd_fluxes (as tests/test_config1_scalar_transport.py takes them)
  Tf, phiTf = qgdFlux         numpy: linear, or `Gauss upwind` phiu (pos0(phiu) (T_O - T_N) + T_N) inside, the patch value on patch faces
  the matrix and the source   numpy from mesh.array(...): Euler ddt, surfaceIntegrate, a_f = Hif |Sf| delta_f (nonOrthDeltaCoeffs inside,
                              deltaCoeffs on patches), fixedValue faces add a_b to the diagonal and a_b T_b to the source
  the solve                   scipy.sparse.linalg.spsolve (direct)
  adjustTimeStep              setDeltaT-QGDQHD.H L41-61 evaluated here
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

from qgdsolver_amd import _lib as L

import oracle
from util import oracle_mesh_of

SMALL = 1e-15


def delta_t_rule(dt, max_u_by_h, min_tau, max_co, max_delta_t, c_tau=0.75):
    """(CoNum seen by the control, new deltaT) [scalarTransportQHDFoam.C L88-92, setDeltaT-QGDQHD.H L41-61]"""
    co = dt * max_u_by_h
    fact0 = max_co / (co + SMALL)
    fact = min(min(fact0, 1.0 + 0.1 * fact0), 1.2)
    return co, min(fact * dt, min(max_delta_t, c_tau * min_tau))


class ScalarRef:
    def __init__(self, mesh, stencil, U, T, bcs, tau, rho0=1.0, mu=0.0, Pr=1.0, upwind=False, implicit=True):
        """bcs: per patch {"U": (word, value), "T": (word, value)}; tau: the uniform tauQGD of constTau / T0byGr"""
        self.mesh, self.stencil, self.upwind, self.implicit = mesh, stencil, upwind, implicit
        self.om = oracle_mesh_of(mesh)
        m = mesh
        self.nif, self.nF, self.nC, self.nb = m.nInternalFaces, m.nFaces, m.nCells, m.nBoundaryFaces
        self.own, self.nei = m.array("owner"), m.array("neighbour")
        self.V, self.w = m.array("V"), m.array("weights")
        Sf = m.array("Sf").reshape(-1, 3)
        magSf = m.array("magSf")
        nif = self.nif
        delta = np.where(np.arange(self.nF) < nif, m.array("nonOrthDeltaCoeffs"), m.array("deltaCoeffs"))
        ps, pz, pt = m.array("patchStart"), m.array("patchSize"), m.array("patchType")
        self.live = np.ones(self.nF, dtype=bool)          # faces that carry a field (not on empty patches)
        self.fixedT = np.zeros(self.nb, dtype=bool)
        self.Tfixed = np.zeros(self.nb)
        U = np.asarray(U, dtype=np.float64).reshape(-1, 3)
        Ub = np.zeros((self.nb, 3))
        for i in range(m.nPatches):
            fs = np.arange(int(ps[i]), int(ps[i]) + int(pz[i]))
            b = fs - nif
            if int(pt[i]) == L.PATCH_EMPTY:
                self.live[fs] = False
                continue
            uo = U[self.own[fs]]
            kind, val = bcs[i]["U"]
            if int(pt[i]) in (L.PATCH_SYMMETRYPLANE, L.PATCH_SYMMETRY):
                kind = "slip"
            if kind == "fixedValue":
                Ub[b] = np.asarray(val, dtype=np.float64)
            elif kind == "slip":                          # basicSymmetry: (pif + transform(I - 2 nn, pif))/2 = pif - n (n & pif)
                n = Sf[fs] / magSf[fs][:, None]
                Ub[b] = uo - n * (n * uo).sum(axis=1)[:, None]
            else:
                Ub[b] = uo
            kind, val = bcs[i]["T"]
            if kind == "fixedValue" and int(pt[i]) == L.PATCH_GENERIC:
                self.fixedT[b] = True
                self.Tfixed[b] = float(val)
        self.U = (U, Ub)
        self.rho = (np.full(self.nC, rho0), np.full(self.nb, rho0))
        self.tau = np.full(self.nF, float(tau))
        self.T = np.array(T, dtype=np.float64).reshape(-1)
        Hi = (mu / Pr) / rho0
        self.a = np.where(self.live, Hi * magSf * delta, 0.0)
        # the matrix without fvm::ddt: -fvm::laplacian(Hif, T)
        own, nei, a = self.own, self.nei, self.a
        diag = np.zeros(self.nC)
        np.add.at(diag, own[:nif], a[:nif]); np.add.at(diag, nei, a[:nif])
        ab = np.where(self.fixedT, a[nif:], 0.0)
        np.add.at(diag, own[nif:], ab)
        self.diagL = diag
        self.off = sp.coo_matrix((np.concatenate([-a[:nif], -a[:nif]]), (np.concatenate([own[:nif], nei]), np.concatenate([nei, own[:nif]]))),
                                 shape=(self.nC, self.nC)).tocsr()
        self.srcB = np.zeros(self.nC)
        np.add.at(self.srcB, own[nif:], ab * self.Tfixed)
        self.time, self.steps = 0.0, 0
        fl = self.fluxes()
        self.phiu = fl["phiu"]
        self.divPhiu = self.div(self.phiu)
        Ufm = np.zeros((self.nF, 3))
        Ufm[:nif] = self.w[:nif, None] * (U[own[:nif]] - U[nei]) + U[nei]
        Ufm[nif:] = Ub
        self.Uf = np.where(self.live[:, None], Ufm, 0.0)

    def Tb(self):
        return np.where(self.fixedT, self.Tfixed, self.T[self.own[self.nif:]])

    def fluxes(self):
        """phiu, gradTf, phiTauTReg of the current T, and phiTf = qgdFlux(phiu, T, Tf)"""
        out = oracle.qhd_fluxes(self.om, self.stencil, self.U, (self.T, self.Tb()), self.rho, self.tau, 0.0, (0, 0, 0))
        nif, own, nei, T = self.nif, self.own, self.nei, self.T
        phiu = out["phiu"]
        Tf = np.zeros(self.nF)
        if self.upwind:
            pos = (phiu[:nif] >= 0.0).astype(np.float64)
            Tf[:nif] = pos * (T[own[:nif]] - T[nei]) + T[nei]
        else:
            Tf[:nif] = self.w[:nif] * (T[own[:nif]] - T[nei]) + T[nei]
        Tf[nif:] = self.Tb()
        out["phiTf"] = np.where(self.live, phiu * Tf, 0.0)
        return out

    def div(self, phi):
        """surfaceIntegrate times V"""
        nif = self.nif
        d = np.zeros(self.nC)
        np.add.at(d, self.own[:nif], phi[:nif]); np.subtract.at(d, self.nei, phi[:nif])
        np.add.at(d, self.own[nif:], np.where(self.live[nif:], phi[nif:], 0.0))
        return d

    def step(self, dt):
        self.time += dt
        self.steps += 1
        if not self.implicit:        # the listing has no else: T is left as it is
            return
        fl = self.fluxes()
        rhs = self.V / dt * self.T - self.div(fl["phiTf"]) + self.divPhiu * self.T + self.div(fl["phiTauTReg"]) + self.srcB
        A = (self.off + sp.diags(self.V / dt + self.diagL)).tocsc()
        self.T = spsolve(A, rhs)
