"""Host replay of a QGDFoam case that carries species (not a test): the species block of reactingLagrangianQGDFoam
[reactingLagrangianQGDFoam.C L92-140] around an OracleCase, out of the oracle's stateless species operators.

Per step: updateFluxes() materialises the face fields of the state before the step; qgdfoam.speciesFlux per transported species
[updateFluxes.H L117-132; the inert one gets no flux, its diffusiveFlux is cleared, L103-116]; step(1) advances the flow (QGDRhoEqn,
QGDUEqn, QGDEEqn); qgdfoam.QGDYEqn [QGDYEqn.H L38-92] with the old and the new density and that step's deltaT; the patch values
follow the species' boundary conditions (zeroGradient: the owner's value, fixedValue: its value).

An updateFluxes() between steps must not change the oracle's trajectory: tests/test_species_case.py checks that bit for bit on the meshes
it uses.  With qgdFlux walls it does (updateFluxes re-evaluates p's boundary condition from the fresh phiwStar): there the face fields are
read from a SECOND oracle case brought to the same state -- ``fresh()`` returns a new case at the initial state, which is stepped as far as
the main one and then asked for its fluxes -- and the main case only ever sees step().
"""
import numpy as np

from qgdsolver_amd import qgdfoam

import oracle as orc


class HostDev:
    def __init__(self, mesh):
        self.mesh = mesh


def patch_values(mesh, Yc, bcs):
    """patch values of one species: bcs = {patch: ("fixedValue", value)}; every other patch takes the owner's value"""
    nif = mesh.nInternalFaces
    own = mesh.array("owner")
    Yb = np.array(Yc[own[nif:]], dtype=float)
    start, size = mesh.array("patchStart"), mesh.array("patchSize")
    for patch, (kind, value) in (bcs or {}).items():
        if kind == "fixedValue":
            Yb[start[patch] - nif:start[patch] - nif + size[patch]] = float(value)
    return Yb


class SpeciesReplay:
    def __init__(self, mesh, omesh, ocase, scheme, Y0, inert, ScNumbers=None, bcs=None, fresh=None):
        """Y0: list of cell fields; bcs: per species a dict {patch: (kind, value)} (or None); fresh: None, or a callable that returns a
        new OracleCase at the state ocase was created with (the face fields are then read from such a case, not from ocase)"""
        self.fresh, self.steps = fresh, 0
        self.mesh, self.om, self.oc, self.scheme = mesh, omesh, ocase, scheme
        self.n = len(Y0)
        self.inert = int(inert)
        self.Sc = [1.0] * self.n if ScNumbers is None else [float(s) for s in ScNumbers]
        self.bcs = bcs if bcs is not None else [None] * self.n
        self.Y = [np.array(y, dtype=float) for y in Y0]
        self.Yb = [patch_values(mesh, self.Y[i], self.bcs[i]) for i in range(self.n)]
        self.phiJmY = [np.zeros(mesh.nFaces) for _ in range(self.n)]
        self.diffusiveFlux = [np.zeros(mesh.nFaces) for _ in range(self.n)]
        self.deltaT = None

    def _flux_call(self, *a):
        assert orc.species_flux(self.om, *a) == 0

    def _step_call(self, *a):
        assert orc.species_step(self.om, *a) == 0

    def step(self, n=1):
        oc, dev = self.oc, HostDev(self.mesh)
        for _ in range(n):
            src = oc
            if self.fresh is not None:
                src = self.fresh()
                if self.steps:
                    src.step(self.steps)
                assert np.array_equal(src.field("rho"), oc.field("rho")) and src.info()["deltaT"] == oc.info()["deltaT"]
            src.updateFluxes()
            phiJm, phi, tau, muf = src.field("phiJm"), src.field("phi"), src.field("tauQGDf"), src.field("muf")
            rho_old = src.field("rho")
            U = (src.field("U"), src.field("U.boundary"))
            if src is not oc:
                src.close()
            self.diffusiveFlux[self.inert] = np.zeros(self.mesh.nFaces)           # updateFluxes.H L103-116
            for i in range(self.n):
                if i == self.inert:
                    continue
                r = qgdfoam.speciesFlux(dev, self.scheme, (self.Y[i], self.Yb[i]), U, phiJm, phi, tau, call=self._flux_call)
                self.phiJmY[i], self.diffusiveFlux[i] = r["phiJmY"], r["diffusiveFlux"]
            oc.step(1)
            rho = oc.field("rho")
            self.deltaT = oc.info()["deltaT"]
            self.steps += 1
            pairs = [(self.Y[i], self.Yb[i]) for i in range(self.n)]
            self.Y = qgdfoam.QGDYEqn(dev, pairs, rho_old, rho, self.phiJmY, muf, self.Sc, self.deltaT, self.diffusiveFlux, self.inert,
                                     call=self._step_call)
            self.Yb = [patch_values(self.mesh, self.Y[i], self.bcs[i]) for i in range(self.n)]
        return self.Y
