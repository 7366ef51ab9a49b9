"""Host replay of a QGDFoam case that carries species on the implicitDiffusion branch (not a test): tests/species_ref.py's replay with its
step ending in QGDYEqn.H L47-66 -- qgdfoam.QGDYEqn(implicitDiffusion=True) over the oracle's stateless implicit species operator
(orc.species_step_implicit), with masks of each species' fixedValue patch faces, the old and the new density and that step's deltaT.

The OracleCase is created with implicitDiffusion=1; the face fields come from a ``fresh()`` case, as the explicit replay does for qgdFlux
walls (an updateFluxes() between steps must not move the main case's trajectory)."""
import numpy as np

from qgdsolver_amd import qgdfoam

import oracle as orc
from species_ref import HostDev, SpeciesReplay, patch_values


def fixed_value_masks(mesh, bcs):
    """per species a uint8 mask over the boundary faces: 1 on the faces of its fixedValue patches"""
    nif = mesh.nInternalFaces
    start, size = mesh.array("patchStart"), mesh.array("patchSize")
    masks = []
    for b in bcs:
        m = np.zeros(mesh.nBoundaryFaces, dtype=np.uint8)
        for patch, (kind, _) in (b or {}).items():
            if kind == "fixedValue":
                m[start[patch] - nif:start[patch] - nif + size[patch]] = 1
        masks.append(m)
    return masks


class SpeciesImplicitReplay(SpeciesReplay):
    def __init__(self, mesh, omesh, ocase, scheme, Y0, inert, ScNumbers=None, bcs=None, fresh=None, tolerance=1e-14, maxIter=2000):
        assert fresh is not None
        super().__init__(mesh, omesh, ocase, scheme, Y0, inert, ScNumbers=ScNumbers, bcs=bcs, fresh=fresh)
        self.tolerance, self.maxIter = float(tolerance), int(maxIter)
        self.fixed = fixed_value_masks(mesh, self.bcs)
        self.muf = None          # muf of the state before the last step (the sign test restates YEqn.flux() from it)
        self.explicitFlux = None  # diffusiveFlux_i as updateFluxes.H left it in the last step, before YEqn.flux() was added

    def _step_call(self, *a):
        assert orc.species_step_implicit(self.om, *a) == 0

    def step(self, n=1):
        oc, dev = self.oc, HostDev(self.mesh)
        for _ in range(n):
            src = self.fresh()
            if self.steps:
                src.step(self.steps)
            assert np.array_equal(src.field("rho"), oc.field("rho")) and src.info()["deltaT"] == oc.info()["deltaT"]
            src.updateFluxes()
            phiJm, phi, tau, muf = src.field("phiJm"), src.field("phi"), src.field("tauQGDf"), src.field("muf")
            rho_old = src.field("rho")
            U = (src.field("U"), src.field("U.boundary"))
            src.close()
            self.diffusiveFlux[self.inert] = np.zeros(self.mesh.nFaces)           # updateFluxes.H L103-116
            for i in range(self.n):
                if i == self.inert:
                    continue
                r = qgdfoam.speciesFlux(dev, self.scheme, (self.Y[i], self.Yb[i]), U, phiJm, phi, tau, call=self._flux_call)
                self.phiJmY[i], self.diffusiveFlux[i] = r["phiJmY"], r["diffusiveFlux"]
            self.muf = muf
            self.explicitFlux = [np.array(d) for d in self.diffusiveFlux]
            oc.step(1)
            rho = oc.field("rho")
            self.deltaT = oc.info()["deltaT"]
            self.steps += 1
            pairs = [(self.Y[i], self.Yb[i]) for i in range(self.n)]
            self.Y = qgdfoam.QGDYEqn(dev, pairs, rho_old, rho, self.phiJmY, muf, self.Sc, self.deltaT, self.diffusiveFlux, self.inert,
                                     implicitDiffusion=True, fixedValueFaces=self.fixed, tolerance=self.tolerance, maxIter=self.maxIter,
                                     call=self._step_call)
            self.Yb = [patch_values(self.mesh, self.Y[i], self.bcs[i]) for i in range(self.n)]
        return self.Y
