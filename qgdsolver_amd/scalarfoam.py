"""scalarTransportQHDFoam resident on the device: createFields.H + the while-loop body of scalarTransportQHDFoam.C L86-125 over the
C-ABI (qgd_scalar_case_*).

U is read and never advanced and thermo.correct() runs once, so ``set_fields`` forms everything that does not depend on T (Uf, phiu,
tauQGDf phiu Uf, the matrix of fvm::laplacian(Hif, T), div(phiu)); ``step`` is then patch and vertex values of T, one face kernel, one
cell kernel and the solve.  With ``implicitDiffusion=0`` the listing leaves T unchanged and only advances time; so does ``step``.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .qgdfoam import STENCIL_IDS
from .qhdfoam import TAU_MODELS

_BC = {"zeroGradient": L.BC_ZEROGRADIENT, "fixedValue": L.BC_FIXEDVALUE, "slip": L.BC_SLIP, "none": L.BC_NONE}
_FLUX = {"linear": L.FLUX_LINEAR, "upwind": L.FLUX_UPWIND}
_FACE_FIELDS = {"phiu": 1, "phiTf": 1, "phiTauTReg": 1, "tauQGDf": 1, "hQGDf": 1, "gradTf": 3, "Uf": 3}


def scalar_options(**kw):
    """qgd_scalar_options with the library defaults; stencil, tauModel and fluxSchemeT may be given as words"""
    o = L.ScalarOptions()
    L.check(L.lib.qgd_scalar_options_default(C.byref(o)), "qgd_scalar_options_default")
    for k, v in kw.items():
        if k == "stencil" and isinstance(v, str):
            v = STENCIL_IDS[v]
        if k == "tauModel" and isinstance(v, str):
            v = TAU_MODELS[v]
        if k == "fluxSchemeT" and isinstance(v, str):
            v = _FLUX[v]
        if not hasattr(o, k):
            raise AttributeError(f"qgd_scalar_options has no member '{k}'")
        setattr(o, k, v)
    return o


class ScalarTransportQHDCase:
    """one scalar T carried by a frozen velocity field: fvm::ddt(T) + fvc::div(phiTf) - fvc::Sp(fvc::div(phiu),T) - fvm::laplacian(Hif,T)
    - fvc::div(phiTauTReg) == 0, one device"""

    def __init__(self, dev, options=None):
        self.dev, self.mesh = dev, dev.mesh
        self.options = options if options is not None else scalar_options()
        h = C.c_void_p()
        L.check(L.lib.qgd_scalar_case_create(dev._h, C.byref(self.options), C.byref(h)), "qgd_scalar_case_create")
        self._handle = L.NativeHandle(h, L.lib.qgd_scalar_case_free)
        dev.adopt(self._handle)

    def set_bc(self, patch, U=("zeroGradient", None), T=("zeroGradient", None)):
        """U: zeroGradient | fixedValue (vector) | slip; T: zeroGradient | fixedValue (scalar).  A word the case does not know reaches the
        library as an invalid kind and comes back as ERR_INVALID."""
        vu = np.asarray(U[1] if U[1] is not None else (0.0, 0.0, 0.0), dtype=np.float64)
        L.check(L.lib.qgd_scalar_case_set_bc(self._h, int(patch), _BC.get(U[0], -1), vu.ctypes.data_as(L.c_double_p), _BC.get(T[0], -1),
                                             float(T[1] or 0.0)), f"qgd_scalar_case_set_bc(U {U[0]}, T {T[0]})")

    def set_fields(self, U, T):
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (U, T)]
        assert a[0].size == 3 * self.mesh.nCells and a[1].size == self.mesh.nCells
        L.check(L.lib.qgd_scalar_case_set_fields(self._h, *[x.ctypes.data_as(L.c_double_p) for x in a]), "qgd_scalar_case_set_fields")

    def step(self, n=1):
        L.check(L.lib.qgd_scalar_case_step(self._h, int(n)), "qgd_scalar_case_step")

    def field(self, name):
        """T, T.boundary; face fields phiu, tauQGDf, hQGDf, Uf and -- formed from the current T -- gradTf, phiTf, phiTauTReg"""
        nc = _FACE_FIELDS.get(name, 1)
        n = self.mesh.nFaces if name in _FACE_FIELDS else (self.mesh.nBoundaryFaces if name.endswith(".boundary") else self.mesh.nCells)
        out = np.zeros((n, nc) if nc > 1 else (max(n, 1),))
        L.check(L.lib.qgd_scalar_case_get_field(self._h, name.encode(), out.ctypes.data_as(L.c_double_p), out.size), f"qgd_scalar_case_get_field({name})")
        return out if nc > 1 else out[:n]

    def info(self):
        a = (C.c_double * 12)()
        L.check(L.lib.qgd_scalar_case_info(self._h, a), "qgd_scalar_case_info")
        return dict(time=a[0], deltaT=a[1], CoNum=a[2], steps=int(a[3]), iterations=int(a[4]), initialResidual=a[5], finalResidual=a[6],
                    unconverged_steps=int(a[7]), stalled_steps=int(a[8]), solver={0: None, 1: "pcg", 2: "chebyshev"}[int(a[9])],
                    maxUbyH=a[10], minTau=a[11])

    def sync(self):
        L.check(L.lib.qgd_scalar_case_sync(self._h), "qgd_scalar_case_sync")

    @property
    def _h(self):
        return self._handle.value

    def close(self):
        if getattr(self, "_handle", None):
            self._handle.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
