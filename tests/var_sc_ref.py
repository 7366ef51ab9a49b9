"""numpy restatement of the varScModel7 pressure-jump sensor [varScModel7.C L166-254], the reference of the device kernel's tests.

Per cell, over its faces:  internal face: sumpf += linearInterpolate(p), sumDpF += r_f (p_other - p_self);  patch face (empty and
wedge patches skipped): sumpf += p_b, sumDpF += r_b (p_b - p_self);  ScQGD = cSc1 |sumDpF| / (sumpf / n), then the two clips and the
cells of constScCellSet.  r_f = nonOrthDeltaCoeff / deltaCoeff with the library's L0 readings: fvc::snGrad is the `reduced` stencil's,
1 / max(n.d, 0.05 |d|); deltaCoeffs = 1 / |d|, d = C_N - C_O (internal), Cf - C_O (patch); the patch snGrad coefficient is 1 / |n.d|."""
import numpy as np

from qgdsolver_amd import _lib as L


class SensorGeometry:
    """r_f, w and the empty / wedge mask out of a PolyMesh's arrays"""

    def __init__(self, mesh):
        nif = mesh.nInternalFaces
        self.nC, self.nif = mesh.nCells, nif
        own = mesh.array("owner").astype(np.int64)
        self.own_i, self.nei, self.own_b = own[:nif], mesh.array("neighbour").astype(np.int64)[:nif], own[nif:]
        Sf = mesh.array("Sf").reshape(-1, 3)
        n = Sf / np.linalg.norm(Sf, axis=1)[:, None]
        C, Cf = mesh.array("C").reshape(-1, 3), mesh.array("Cf").reshape(-1, 3)
        d = C[self.nei] - C[self.own_i]
        magd = np.linalg.norm(d, axis=1)
        self.r_i = magd / np.maximum((n[:nif] * d).sum(axis=1), 0.05 * magd)
        db = Cf[nif:] - C[self.own_b]
        self.w = mesh.array("weights")[:nif]
        self.keep = np.ones(mesh.nBoundaryFaces, dtype=bool)
        ps, pz, pt = mesh.array("patchStart"), mesh.array("patchSize"), mesh.array("patchType")
        for i in range(mesh.nPatches):
            if int(pt[i]) in (L.PATCH_EMPTY, L.PATCH_WEDGE):
                self.keep[int(ps[i]) - nif: int(ps[i]) - nif + int(pz[i])] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            self.r_b = np.where(self.keep, np.linalg.norm(db, axis=1) / np.abs((n[nif:] * db).sum(axis=1)), 0.0)


def sensor(geo, p, pb, ScQGD, cSc1=1.0, minSc=-1.0, maxSc=-1.0, const_cells=None):
    """(ScQGD of the cells, ScQGD of the patch faces) from the cell pressures p and the patch pressures pb"""
    p, pb = np.asarray(p, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    sum_dp, sum_p, cnt = np.zeros(geo.nC), np.zeros(geo.nC), np.zeros(geo.nC)
    pf = geo.w * p[geo.own_i] + (1.0 - geo.w) * p[geo.nei]
    dpf = geo.r_i * (p[geo.nei] - p[geo.own_i])
    np.add.at(sum_dp, geo.own_i, dpf)
    np.add.at(sum_dp, geo.nei, -dpf)
    for cells in (geo.own_i, geo.nei):
        np.add.at(sum_p, cells, pf)
        np.add.at(cnt, cells, 1.0)
    k, ob = geo.keep, geo.own_b
    np.add.at(sum_dp, ob[k], geo.r_b[k] * (pb[k] - p[ob[k]]))
    np.add.at(sum_p, ob[k], pb[k])
    np.add.at(cnt, ob[k], 1.0)
    sc = cSc1 * np.abs(sum_dp) / (sum_p / cnt)
    scb = np.full(pb.shape, float(ScQGD))
    if minSc >= 0:
        sc, scb = np.maximum(sc, minSc), np.maximum(scb, minSc)
    if maxSc >= 0:
        sc, scb = np.minimum(sc, maxSc), np.minimum(scb, maxSc)
    if const_cells is not None and len(const_cells):
        sc[np.asarray(const_cells, dtype=np.int64)] = ScQGD
    return sc, scb
