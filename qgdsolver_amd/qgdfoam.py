"""Host-side mirror of the QGDFoam loop pieces over the C-ABI.

``QGDFoamCase`` holds what createFields.H / createFaceFields.H / createFaceFluxes.H
create; ``updateFluxes()`` is updateFields.H + updateFluxes.H; ``step()`` is the
``while (runTime.run())`` body (QGDFoam.C L90-163).  ``thermo`` exposes the
QGDThermo accessor names (QGDThermo.H L99-135).
"""
import ctypes as C

import numpy as np

from . import _lib as L

_VECTOR_FIELDS = {"U": 3, "rhoU": 3, "phiJmU": 3, "phiP": 3, "phiPi": 3, "gradUf": 9, "gradef": 3, "gradRhof": 3, "gradPf": 3, "phiTauMC": 3}
_FACE_FIELDS = {"phiJm", "phiJmU", "phiP", "phiPi", "phiJmH", "phiQ", "phiPiU", "phiwStar", "phi", "tauQGDf", "hQGDf",
                "gradUf", "gradef", "gradRhof", "gradPf", "phiTauMC", "phiSigmaDotU"}

STENCIL_IDS = {"reduced": L.FVSC_REDUCED, "leastSquares": L.FVSC_LEASTSQUARES, "leastSquaresOpt": L.FVSC_LEASTSQUARES,
               "GaussVolPoint": L.FVSC_GAUSSVOLPOINT}


TERM_ORDER = ("grad(U)", "grad(e)", "grad(rho)", "grad(p)")   # qgd_case_options::termStencil [QGDFoam/updateFluxes.H L41-65]


def default_options(**kw):
    """qgd_case_options with the library defaults.  ``stencil`` may be a word; ``termStencils`` a dict {"grad(p)": "reduced", ...} of
    per-term fvsc entries [fvsc.C L51-58] (terms not named take ``stencil``)"""
    o = L.CaseOptions()
    L.check(L.lib.qgd_case_options_default(C.byref(o)), "qgd_case_options_default")
    for k, v in kw.items():
        if k == "stencil" and isinstance(v, str):
            v = STENCIL_IDS[v]
        if k == "termStencils":
            for term, word in (v or {}).items():
                o.termStencil[TERM_ORDER.index(term)] = 1 + (STENCIL_IDS[word] if isinstance(word, str) else int(word))
            continue
        if k == "varSc":     # the varScModel7 entries of foamfile.read_case_setup: they go to QGDFoamCase.set_var_sc
            continue
        if k == "species":   # the species entries of foamfile.read_case_setup: they go to QGDFoamCase.set_species
            continue
        setattr(o, k, v)
    return o


class QGDThermo:
    """Accessor surface of QGDThermo (QGDThermo.H L99-135)."""

    def __init__(self, case):
        self._c = case

    def tauQGDf(self):
        return self._c.field("tauQGDf")

    def hQGDf(self):
        return self._c.field("hQGDf")

    def tauQGD(self):
        return self._c.field("tauQGD")

    def hQGD(self):
        return self._c.field("hQGD")

    def muQGD(self):
        return self._c.field("muQGD")

    def alphauQGD(self):
        return self._c.field("alphauQGD")

    def c(self):
        return self._c.field("c")

    def p(self):
        return self._c.field("p")

    def rho(self):
        return self._c.field("rho")

    def mu(self):
        return self._c.field("mu")

    def implicitDiffusion(self):
        return bool(self._c.options.implicitDiffusion)


class QGDFoamCase:
    def __init__(self, dev, options=None):
        self.dev = dev
        self.mesh = dev.mesh
        self.options = options if options is not None else default_options()
        h = C.c_void_p()
        L.check(L.lib.qgd_case_create(dev._h, C.byref(self.options), C.byref(h)), "qgd_case_create")
        self._handle = L.NativeHandle(h, L.lib.qgd_case_free)
        dev.adopt(self._handle)
        self._monitor_handles = []
        self.thermo = QGDThermo(self)

    def set_bc(self, patch, U=("zeroGradient", None), T=("zeroGradient", None), p=("zeroGradient", None)):
        kinds = {"zeroGradient": L.BC_ZEROGRADIENT, "fixedValue": L.BC_FIXEDVALUE, "slip": L.BC_SLIP, "qgdFlux": L.BC_QGDFLUX,
                 "none": L.BC_NONE}
        # a fixedValue entry takes the patch's one value ((3,) for U, a float for T and p) or one value per face of the patch on this
        # device's mesh ((nFaces, 3), (nFaces,)): qgd_case_set_bc_values, after the entry itself
        lists = {}
        for field, entry in (("U", U), ("T", T), ("p", p)):
            if entry[1] is not None and np.ndim(entry[1]) == (2 if field == "U" else 1):
                if entry[0] != "fixedValue":
                    raise ValueError(f"set_bc: {field} of patch {patch}: a value list belongs to a fixedValue entry, not to '{entry[0]}'")
                lists[field] = np.ascontiguousarray(entry[1], dtype=np.float64)
        one = lambda field, entry: 0.0 if field in lists else float(entry[1] or 0.0)   # noqa: E731
        vu = np.asarray(U[1] if (U[1] is not None and "U" not in lists) else (0.0, 0.0, 0.0), dtype=np.float64)
        L.check(L.lib.qgd_case_set_bc(self._h, patch, kinds[U[0]], vu.ctypes.data_as(L.c_double_p), kinds[T[0]],
                                      one("T", T), kinds[p[0]], one("p", p)), "qgd_case_set_bc")
        for field, values in lists.items():
            self.set_bc_values(patch, field, values)

    _BC_FIELDS = {"U": 0, "T": 1, "p": 2}

    def set_bc_values(self, patch, field, values):
        """one value per face of a fixedValue entry (qgd_case_set_bc_values): field "U" (nFaces, 3), "T" / "p" (nFaces,), in the patch's
        face order on this device's mesh; None drops the list (the entry reads its uniform value again).  Before set_fields."""
        k = self._BC_FIELDS[field]
        if values is None:
            L.check(L.lib.qgd_case_set_bc_values(self._h, int(patch), k, None, 0), "qgd_case_set_bc_values")
            return
        a = np.ascontiguousarray(values, dtype=np.float64)
        if a.ndim != (2 if k == 0 else 1) or (k == 0 and a.shape[1] != 3):
            raise ValueError(f"set_bc_values: {field} takes an array of shape {'(nFaces, 3)' if k == 0 else '(nFaces,)'}, got {a.shape}")
        buf = a if a.size else np.zeros(3)
        L.check(L.lib.qgd_case_set_bc_values(self._h, int(patch), k, buf.ctypes.data_as(L.c_double_p), int(a.shape[0])), "qgd_case_set_bc_values")

    def get_bc_values(self, patch, field):
        """(what a fixedValue entry prescribes per face of the patch, whether it is a value list) -- qgd_case_get_bc_values"""
        k = self._BC_FIELDS[field]
        n = int(self.mesh.array("patchSize")[patch])
        out = np.zeros((n, 3) if k == 0 else (n,))
        buf = out if out.size else np.zeros(3)
        is_list = C.c_int32()
        L.check(L.lib.qgd_case_get_bc_values(self._h, int(patch), k, buf.ctypes.data_as(L.c_double_p), n, C.byref(is_list)), "qgd_case_get_bc_values")
        return out, bool(is_list.value)

    def set_fields(self, U, T, p):
        U = np.ascontiguousarray(U, dtype=np.float64)
        T = np.ascontiguousarray(T, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert U.size == 3 * self.mesh.nCells and T.size == self.mesh.nCells and p.size == self.mesh.nCells
        L.check(L.lib.qgd_case_set_fields(self._h, U.ctypes.data_as(L.c_double_p), T.ctypes.data_as(L.c_double_p),
                                          p.ctypes.data_as(L.c_double_p)), "qgd_case_set_fields")

    def set_qgd_coeffs(self, alphaQGD=None, ScQGD=None):
        """non-uniform alphaQGD / ScQGD fields (QGDCoeffs.C L119-160, constScPrModel1.C L66-79): each a pair
        (cell values, patch values) or None for the uniform value of the options; call before set_fields"""
        keep = []

        def ptrs(pair):
            if pair is None:
                return None, None
            c = np.ascontiguousarray(pair[0], dtype=np.float64)
            b = np.ascontiguousarray(pair[1], dtype=np.float64)
            assert c.size == self.mesh.nCells and b.size == self.mesh.nBoundaryFaces
            if b.size == 0:
                b = np.zeros(1)
            keep.extend([c, b])
            return c.ctypes.data_as(L.c_double_p), b.ctypes.data_as(L.c_double_p)

        a, ab = ptrs(alphaQGD)
        s, sb = ptrs(ScQGD)
        L.check(L.lib.qgd_case_set_qgd_coeffs(self._h, a, ab, s, sb), "qgd_case_set_qgd_coeffs")

    def set_var_sc(self, model="varScModel7", ScQGD=None, cSc1=1.0, minSc=-1.0, maxSc=-1.0, const_cells=None):
        """the varScModel7 closure (varScModel7.C L166-300; qgd_case_set_var_sc): ScQGD per cell from the pressure jumps across the
        cell's faces, cSc1 |sum r_f dp| / mean p_f, clipped to [minSc, maxSc] where those are >= 0, ``ScQGD`` itself on the cells of
        ``const_cells`` (labels of this device's mesh) and on the patches.  model None: back to the uniform ScQGD.  Before set_fields."""
        if model is None:
            L.check(L.lib.qgd_case_set_var_sc(self._h, None, None), "qgd_case_set_var_sc")
            return
        if ScQGD is None:
            raise ValueError("set_var_sc: ScQGD (the dictionary's mandatory entry) is missing")
        cells = np.ascontiguousarray(const_cells if const_cells is not None else [], dtype=np.int32).reshape(-1)
        o = L.VarScOptions()
        # another word travels as model 0, which the library refuses by name
        o.model = 7 if model in ("varScModel7", 7) else (int(model) if isinstance(model, (int, np.integer)) else 0)
        o.nConstCells = int(cells.size)
        o.ScQGD, o.cSc1, o.minSc, o.maxSc = float(ScQGD), float(cSc1), float(minSc), float(maxSc)
        L.check(L.lib.qgd_case_set_var_sc(self._h, C.byref(o), cells.ctypes.data_as(L.c_int32_p) if cells.size else None), "qgd_case_set_var_sc")

    def sc_range(self):
        """(max, min) of ScQGD over the owned cells: the reference's ``max/min ScQGD`` line (qgd_case_sc_range)"""
        a = (C.c_double * 2)()
        L.check(L.lib.qgd_case_sc_range(self._h, a), "qgd_case_sc_range")
        return a[0], a[1]

    # ---- species mass fractions advanced with the flow (qgd_case_set_species; passive composition: one thermo, no chemistry) ----
    def set_species(self, names, inert, ScNumbers=None, keep_fluxes=False, implicit=False, halo=False):
        """the case carries the mass fractions ``names`` (reactingLagrangianQGDFoam's species block: updateFluxes.H L103-132, QGDYEqn.H
        L38-92, the branch of the case's implicitDiffusion); ``inert`` (a name or an index) is the species that takes 1 - sum of the others; ScNumbers a dict
        {name: Sc} or a sequence (default 1); keep_fluxes keeps phiJmY / diffusiveFlux of the last step for species_field; implicit accepts
        the implicitDiffusion branch (QGD_SPECIES_IMPLICIT: one linear solve per batch of species inside the step; without it a case created
        with implicitDiffusion=1 refuses species, as it always did); halo accepts a sharded or periodic device (QGD_SPECIES_HALO: the state
        message then carries the composition, 8 + nSpecies doubles per cell -- halo_count says so; explicit branch only).  After
        creation, before set_fields.  The case then steps with the separate kernels (fused_info)."""
        names = [str(n) for n in names]
        if len(set(names)) != len(names):
            raise ValueError(f"set_species: species names repeat: {names}")
        k = names.index(inert) if isinstance(inert, str) else int(inert)
        if isinstance(ScNumbers, dict):
            sc = np.array([float(ScNumbers.get(n, 1.0)) for n in names])
        else:
            sc = np.ones(len(names)) if ScNumbers is None else np.ascontiguousarray(ScNumbers, dtype=np.float64).reshape(-1)
        if sc.size != len(names):
            raise ValueError(f"set_species: {len(names)} species, {sc.size} Schmidt numbers")
        buf = sc if sc.size else np.ones(1)
        L.check(L.lib.qgd_case_set_species(self._h, len(names), k, buf.ctypes.data_as(L.c_double_p),
                                           (L.SPECIES_KEEP_FLUXES if keep_fluxes else 0) | (L.SPECIES_IMPLICIT if implicit else 0) | (L.SPECIES_HALO if halo else 0)),
                "qgd_case_set_species")
        self.species = names

    def _species_index(self, s):
        if not isinstance(s, str):
            return int(s)
        names = getattr(self, "species", None)
        if names is None:
            raise ValueError("the case carries no species (set_species)")
        return names.index(s)

    def set_species_bc(self, species, patch, entry=("zeroGradient", None)):
        """boundary condition of one species on one patch: ("zeroGradient", None), ("fixedValue", value) or ("none", None)"""
        kinds = {"zeroGradient": L.BC_ZEROGRADIENT, "fixedValue": L.BC_FIXEDVALUE, "none": L.BC_NONE}
        if entry[0] not in kinds:
            raise ValueError(f"set_species_bc: a species takes zeroGradient, fixedValue or none, not '{entry[0]}'")
        L.check(L.lib.qgd_case_set_species_bc(self._h, self._species_index(species), int(patch), kinds[entry[0]], float(entry[1] or 0.0)),
                "qgd_case_set_species_bc")

    def set_species_field(self, species, Y):
        Y = np.ascontiguousarray(Y, dtype=np.float64).reshape(-1)
        if Y.size != self.mesh.nCells:
            raise ValueError(f"set_species_field: {Y.size} values for {self.mesh.nCells} cells")
        buf = Y if Y.size else np.zeros(1)
        L.check(L.lib.qgd_case_set_species_fields(self._h, self._species_index(species), buf.ctypes.data_as(L.c_double_p)), "qgd_case_set_species_fields")

    def species_field(self, species, what="Y"):
        """"Y" (cells), "Y.boundary" (patch faces); with keep_fluxes also "phiJmY" and "diffusiveFlux" of the last step (faces, by label)"""
        n = {"Y": self.mesh.nCells, "Y.boundary": self.mesh.nBoundaryFaces}.get(what, self.mesh.nFaces)
        out = np.zeros(max(n, 1))
        L.check(L.lib.qgd_case_get_species_field(self._h, self._species_index(species), what.encode(), out.ctypes.data_as(L.c_double_p), n),
                f"qgd_case_get_species_field({what})")
        return out[:n]

    def species_info(self):
        a = (C.c_int64 * 4)()
        L.check(L.lib.qgd_case_species_info(self._h, a), "qgd_case_species_info")
        return dict(nSpecies=int(a[0]), inertIndex=int(a[1]), batchWidth=int(a[2]), keepFluxes=bool(a[3]), names=list(getattr(self, "species", []) or []))

    def set_species_solver(self, tolerance, maxIter):
        """controls of the species' solves on the implicitDiffusion branch (fvSolution.solvers.<species>; default: the case's implicitTol /
        implicitMaxIter)"""
        L.check(L.lib.qgd_case_set_species_solver(self._h, float(tolerance), int(maxIter)), "qgd_case_set_species_solver")

    def species_implicit_info(self):
        """the species' solves of the last step: {unconvergedSteps, stalledSteps, species: {name: {iterations, initial, final}}} (transported
        species only; the counts have the meaning implicit_info gives them)"""
        names = list(getattr(self, "species", []) or [])
        n = 3 + 3 * len(names)
        a = np.zeros(n)
        L.check(L.lib.qgd_case_species_implicit_info(self._h, a.ctypes.data_as(L.c_double_p), n), "qgd_case_species_implicit_info")
        inert = self.species_info()["inertIndex"]
        return dict(unconvergedSteps=int(a[0]), stalledSteps=int(a[1]),
                    species={s: dict(iterations=int(a[3 + 3 * i]), initial=float(a[4 + 3 * i]), final=float(a[5 + 3 * i]))
                             for i, s in enumerate(names) if i != inert})

    def updateFluxes(self):
        L.check(L.lib.qgd_case_update_fluxes(self._h), "qgd_case_update_fluxes")

    def step(self, n=1):
        """n whole steps of an unsharded case; returns when the device has finished (qgd_case_step)"""
        L.check(L.lib.qgd_case_step(self._h, int(n)), "qgd_case_step")

    def step_phase(self, phase):
        """one stream-ordered phase of a step, no host synchronisation (qgd_case_step_phase): 0 assembly, 1 advance (10 + 11: the boundary
        layer of a shard first), 5 + 6 the assembly split around the mid-step exchange, 3 = one whole step of an unsharded case, 20..35 the
        implicitDiffusion branch; the exchanges between the phases are the caller's (halo.py)"""
        L.check(L.lib.qgd_case_step_phase(self._h, int(phase)), "qgd_case_step_phase")

    def reduction_ptr(self):
        """device pointer of the 2-double {max Cof, -min tauQGDf} buffer (valid between phase 0 and phase 1)"""
        p = C.c_void_p()
        L.check(L.lib.qgd_case_reduction_ptr(self._h, C.byref(p)), "qgd_case_reduction_ptr")
        return p.value

    def set_stream(self, raw_stream):
        """Run on a caller-owned hipStream_t (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        L.check(L.lib.qgd_case_set_stream(self._h, C.c_void_p(raw_stream)), "qgd_case_set_stream")

    def set_halo_stream(self, raw_stream):
        L.check(L.lib.qgd_case_set_halo_stream(self._h, C.c_void_p(raw_stream)), "qgd_case_set_halo_stream")

    def sync(self):
        L.check(L.lib.qgd_case_stream_sync(self._h), "qgd_case_stream_sync")

    def field(self, name):
        base = name[:-len(".boundary")] if name.endswith(".boundary") else name
        nc = _VECTOR_FIELDS.get(base, 1)
        if name.endswith(".boundary"):
            n = self.mesh.nBoundaryFaces
        elif base in _FACE_FIELDS:
            n = self.mesh.nFaces
        else:
            n = self.mesh.nCells
        out = np.zeros((n, nc) if nc > 1 else (n,), dtype=np.float64)
        if n:
            L.check(L.lib.qgd_case_get_field(self._h, name.encode(), out.ctypes.data_as(L.c_double_p), out.size),
                    f"qgd_case_get_field({name})")
        return out

    def monitor(self, probes=None, patches=None, species=False):
        """a run monitor of this case (monitor.Monitor; qgd_monitor_create): volume integrals, extrema with their cells, the first
        non-finite cell, the values at ``probes`` (cell labels of this device's mesh, -1 = not on this rank; PolyMesh.find_cells
        locates points) and the totals of the net face fluxes over ``patches`` (indices of real patches), formed on the device by
        ``sample()`` and fetched by ``read()``.  After set_fields.  The monitor is freed with the case where still open.
        species=True (a case with set_species): every sample also carries, per species, the inert one included, sum rho Y_i V, the
        extrema of Y_i with their cells, Y_i at the probes and the net species flux through each patch (qgd_monitor_enable_species)."""
        from .monitor import Monitor
        m = Monitor(self, probes=probes, patches=patches, species=species)
        self._monitor_handles = [h for h in self._monitor_handles if h.value] + [m._handle]
        return m

    def info(self):
        a = (C.c_double * 6)()
        L.check(L.lib.qgd_case_info(self._h, a), "qgd_case_info")
        return dict(time=a[0], deltaT=a[1], CoNum=a[2], minRho=a[3], minE=a[4], steps=int(a[5]))

    def fused_info(self):
        """whether the case advances with the fused kernel of the explicit step (vertex values, faces and cell update of a block of cells in
        one launch), its blocks, faces computed / cell records staged / vertex values formed per step, LDS bytes (qgd_case_fused_info)"""
        a = (C.c_int64 * 8)()
        L.check(L.lib.qgd_case_fused_info(self._h, a), "qgd_case_fused_info")
        return dict(fused=int(a[0]) == 1, fusedImplicit=int(a[0]) == 2, fusedAdjust=int(a[0]) == 3, blocks=int(a[1]), facesComputed=int(a[2]), ldsBytes=int(a[3]), cellsStaged=int(a[4]),
                    cellsStagedFull=int(a[5]), verticesFormed=int(a[6]), layerBlocks=int(a[7]),
                    packedWeights=bool(a[1]) and self.dev.fused_blocks()["packedWeights"],
                    packedFaces=bool(a[1]) and self.dev.fused_blocks()["packedFaces"],
                    packedGeometry=bool(a[1]) and self.dev.fused_blocks()["packedGeometry"])

    def implicit_info(self):
        """the four linear solves of the implicitDiffusion branch in the last step (qgd_case_implicit_info)"""
        a = (C.c_double * 16)()
        L.check(L.lib.qgd_case_implicit_info(self._h, a), "qgd_case_implicit_info")
        names = ("Ux", "Uy", "Uz", "e")
        return dict(implicit=bool(a[13]), solver={0: None, 1: "pcg", 2: "chebyshev"}[int(a[13])], unconverged_steps=int(a[12]), stalled_steps=int(a[14]),
                    solves={n: dict(iterations=int(a[k]), initial=a[4 + k], final=a[8 + k]) for k, n in enumerate(names)})

    def implicit_apply_time(self, reps=20):
        """measurement: average ms over `reps` launches of the kernel the branch spends most of its time in -- one Chebyshev step of the
        U system (iChebKernel<3,0>) or, with QGD_IMPL_SOLVER=pcg, its matrix product (iApplyKernel<3,1>) -- and its rows"""
        a = (C.c_double * 2)()
        L.check(L.lib.qgd_case_implicit_apply_time(self._h, int(reps), a), "qgd_case_implicit_apply_time")
        return dict(ms=a[0], rows=int(a[1]))

    # ---- the implicitDiffusion branch on shards (phases 20..35 of qgd_case_step_phase; halo.ImplicitStepper drives them) ----
    def implicit_control(self):
        """host copy of the 68-double control block of the solve in flight (slot-major: [slot * 4 + component])"""
        a = np.zeros(68)
        L.check(L.lib.qgd_case_implicit_control(self._h, a.ctypes.data_as(L.c_double_p), 0), "qgd_case_implicit_control")
        return a

    def set_implicit_control(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == 68
        L.check(L.lib.qgd_case_implicit_control(self._h, a.ctypes.data_as(L.c_double_p), 1), "qgd_case_implicit_control")

    def implicit_control_ptr(self):
        p = C.c_void_p()
        L.check(L.lib.qgd_case_implicit_control_ptr(self._h, C.byref(p)), "qgd_case_implicit_control_ptr")
        return p.value

    def implicit_solve_done(self):
        a = (C.c_double * 2)()
        L.check(L.lib.qgd_case_implicit_solve_status(self._h, a), "qgd_case_implicit_solve_status")
        return a[0] != 0.0

    # ---- the message in the middle of the flux assembly (step phases 5 | 6 instead of 0; include/qgd_amd.h) ----
    def needs_mid_exchange(self):
        n = C.c_int32()
        L.check(L.lib.qgd_case_mid_exchange_needed(self._h, C.byref(n)), "qgd_case_mid_exchange_needed")
        return bool(n.value)

    def mid_halo_count(self, slot):
        s, r = C.c_int64(), C.c_int64()
        L.check(L.lib.qgd_case_mid_halo_count(self._h, int(slot), C.byref(s), C.byref(r)), "qgd_case_mid_halo_count")
        return s.value, r.value

    def mid_halo_pack(self, slot, dev_ptr):
        L.check(L.lib.qgd_case_mid_halo_pack(self._h, int(slot), C.c_void_p(dev_ptr)), "qgd_case_mid_halo_pack")

    def mid_halo_unpack(self, slot, dev_ptr):
        L.check(L.lib.qgd_case_mid_halo_unpack(self._h, int(slot), C.c_void_p(dev_ptr)), "qgd_case_mid_halo_unpack")

    def implicit_halo_count(self, slot, kind):
        s, r = C.c_int64(), C.c_int64()
        L.check(L.lib.qgd_case_implicit_halo_count(self._h, int(slot), int(kind), C.byref(s), C.byref(r)), "qgd_case_implicit_halo_count")
        return s.value, r.value

    def implicit_halo_pack(self, slot, kind, dev_ptr):
        L.check(L.lib.qgd_case_implicit_halo_pack(self._h, int(slot), int(kind), C.c_void_p(dev_ptr)), "qgd_case_implicit_halo_pack")

    def implicit_halo_unpack(self, slot, kind, dev_ptr):
        L.check(L.lib.qgd_case_implicit_halo_unpack(self._h, int(slot), int(kind), C.c_void_p(dev_ptr)), "qgd_case_implicit_halo_unpack")

    def halo_buffer(self, n):
        """device buffer of n doubles (released with the device)"""
        return self.dev.alloc(8 * max(int(n), 1))

    # ---- halo ------------------------------------------------------------------
    def halo_count(self, slot):
        """doubles in the message sent to the neighbour behind halo slot ``slot``"""
        n = C.c_int64()
        L.check(L.lib.qgd_case_halo_count(self._h, slot, C.byref(n)), "qgd_case_halo_count")
        return n.value

    def halo_recv_count(self, slot):
        n = C.c_int64()
        L.check(L.lib.qgd_case_halo_recv_count(self._h, slot, C.byref(n)), "qgd_case_halo_recv_count")
        return n.value

    def halo_pack(self, side, dev_ptr):
        L.check(L.lib.qgd_case_halo_pack(self._h, side, C.c_void_p(dev_ptr)), "qgd_case_halo_pack")

    def halo_unpack(self, side, dev_ptr):
        L.check(L.lib.qgd_case_halo_unpack(self._h, side, C.c_void_p(dev_ptr)), "qgd_case_halo_unpack")

    # ---- measurement --------------------------------------------------------------
    def timing(self, enable=True):
        L.check(L.lib.qgd_case_timing(self._h, 1 if enable else 0), "qgd_case_timing")

    def timing_reset(self):
        L.check(L.lib.qgd_case_timing_reset(self._h), "qgd_case_timing_reset")

    def kernel_time(self, k):
        ms = C.c_double()
        n = C.c_int64()
        L.check(L.lib.qgd_case_kernel_time(self._h, k, C.byref(ms), C.byref(n)), "qgd_case_kernel_time")
        return ms.value, n.value

    def device_bytes(self):
        n = C.c_int64()
        L.check(L.lib.qgd_case_device_bytes(self._h, C.byref(n)), "qgd_case_device_bytes")
        return n.value

    @property
    def _h(self):
        return self._handle.value

    def close(self):
        if getattr(self, "_handle", None):
            for h in getattr(self, "_monitor_handles", ()):   # a monitor keeps a pointer to its case: freed before it (NativeHandle: once)
                h.free()
            self._monitor_handles = []
            self._handle.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def speciesFlux(dev, scheme, Y, U, phiJm, phi, tauQGDf, call=None):
    """Species block of reactingLagrangianQGDFoam/updateFluxes.H L117-132 for one species.
    Y, U: (internal, boundary) pairs; returns dict(phiJmY, diffusiveFlux, gradYf)."""
    m = dev.mesh
    a = lambda x, n: np.ascontiguousarray(x, dtype=np.float64).reshape(-1) if n else np.zeros(1)  # noqa: E731
    Yc, Yb, Uc, Ub = a(Y[0], m.nCells), a(Y[1], m.nBoundaryFaces), a(U[0], m.nCells), a(U[1], m.nBoundaryFaces)
    jm, ph, tau = a(phiJm, 1), a(phi, 1), a(tauQGDf, 1)
    assert Yc.size == m.nCells and Uc.size == 3 * m.nCells and jm.size == m.nFaces and ph.size == m.nFaces and tau.size == m.nFaces
    out = dict(phiJmY=np.zeros(m.nFaces), diffusiveFlux=np.zeros(m.nFaces), gradYf=np.zeros((m.nFaces, 3)))
    dp = lambda x: x.ctypes.data_as(L.c_double_p)  # noqa: E731
    if call is None:
        sid = STENCIL_IDS[scheme] if isinstance(scheme, str) else int(scheme)
        L.check(L.lib.qgd_species_flux(dev._h, sid, dp(Yc), dp(Yb), dp(Uc), dp(Ub), dp(jm), dp(ph), dp(tau), dp(out["phiJmY"]),
                                       dp(out["diffusiveFlux"]), dp(out["gradYf"])), "qgd_species_flux")
    else:
        call(scheme, Yc, Yb, Uc, Ub, jm, ph, tau, out["phiJmY"], out["diffusiveFlux"], out["gradYf"])
    return out


def speciesStep(dev, Y, rhoOld, rho, phiJmY, muf, Sc, deltaT, diffusiveFlux, Su=None, call=None):
    """One species of QGDYEqn.H L67-86 (explicit branch; the sources as one explicit field Su or None): returns the new cell values of
    Yi (already clipped at 0) and adds (muf/Sc) snGrad(Yi.old) |Sf| to diffusiveFlux in place.  Y: (internal, boundary) pair."""
    m = dev.mesh
    a = lambda x, n: np.ascontiguousarray(x, dtype=np.float64).reshape(-1) if n else np.zeros(1)  # noqa: E731
    Yc, Yb = a(Y[0], m.nCells), a(Y[1], m.nBoundaryFaces)
    ro, rn, jm, mf = a(rhoOld, 1), a(rho, 1), a(phiJmY, 1), a(muf, 1)
    su = None if Su is None else a(Su, 1)
    assert Yc.size == m.nCells and ro.size == m.nCells and rn.size == m.nCells and jm.size == m.nFaces and mf.size == m.nFaces
    assert isinstance(diffusiveFlux, np.ndarray) and diffusiveFlux.dtype == np.float64 and diffusiveFlux.size == m.nFaces and diffusiveFlux.flags.c_contiguous
    Ynew = np.zeros(m.nCells)
    dp = lambda x: x.ctypes.data_as(L.c_double_p)  # noqa: E731
    if call is None:
        L.check(L.lib.qgd_species_step(dev._h, dp(Yc), dp(Yb), dp(ro), dp(rn), dp(jm), dp(mf), float(Sc), float(deltaT),
                                       dp(su) if su is not None else None, dp(diffusiveFlux), dp(Ynew)), "qgd_species_step")
    else:
        call(Yc, Yb, ro, rn, jm, mf, float(Sc), float(deltaT), su, diffusiveFlux, Ynew)
    return Ynew


def speciesStepImplicit(dev, Y, rhoOld, rho, phiJmY, muf, Sc, deltaT, diffusiveFlux, Su=None, fixedValueFaces=None, tolerance=1e-10, maxIter=1000,
                        call=None):
    """One species of QGDYEqn.H L47-66 (the implicitDiffusion branch: fvm::laplacian(muf/Sc, Yi), diffusiveFlux += YEqn.flux()): returns
    (new cell values of Yi clipped at 0, {iterations, initial, final}).  fixedValueFaces: boolean mask over the boundary faces of the
    fixedValue patches of Yi (their values are Y[1]); all other patch faces are zeroGradient."""
    m = dev.mesh
    a = lambda x, n: np.ascontiguousarray(x, dtype=np.float64).reshape(-1) if n else np.zeros(1)  # noqa: E731
    Yc, Yb = a(Y[0], m.nCells), a(Y[1], m.nBoundaryFaces)
    ro, rn, jm, mf = a(rhoOld, 1), a(rho, 1), a(phiJmY, 1), a(muf, 1)
    su = None if Su is None else a(Su, 1)
    fx = None if fixedValueFaces is None else np.ascontiguousarray(fixedValueFaces, dtype=np.uint8).reshape(-1)
    assert Yc.size == m.nCells and ro.size == m.nCells and rn.size == m.nCells and jm.size == m.nFaces and mf.size == m.nFaces
    assert fx is None or fx.size == m.nBoundaryFaces
    assert isinstance(diffusiveFlux, np.ndarray) and diffusiveFlux.dtype == np.float64 and diffusiveFlux.size == m.nFaces and diffusiveFlux.flags.c_contiguous
    Ynew, info = np.zeros(m.nCells), np.zeros(3)
    dp = lambda x: x.ctypes.data_as(L.c_double_p)  # noqa: E731
    if call is None:
        L.check(L.lib.qgd_species_step_implicit(dev._h, dp(Yc), dp(Yb), fx.ctypes.data_as(C.c_void_p) if fx is not None and fx.size else None, dp(ro),
                                                dp(rn), dp(jm), dp(mf), float(Sc), float(deltaT), dp(su) if su is not None else None,
                                                float(tolerance), int(maxIter), dp(diffusiveFlux), dp(Ynew), dp(info)), "qgd_species_step_implicit")
    else:
        call(Yc, Yb, fx, ro, rn, jm, mf, float(Sc), float(deltaT), su, float(tolerance), int(maxIter), diffusiveFlux, Ynew, info)
    return Ynew, dict(iterations=int(info[0]), initial=float(info[1]), final=float(info[2]))


def QGDYEqn(dev, Y, rhoOld, rho, phiJmY, muf, ScNumbers, deltaT, diffusiveFlux, inertIndex, active=None, Su=None, call=None, implicitDiffusion=False,
            fixedValueFaces=None, tolerance=1e-10, maxIter=1000):
    """QGDYEqn.H L38-92 over all species (implicitDiffusion: L47-66 through speciesStepImplicit, fixedValueFaces[i] = mask of species i's
    fixedValue patch faces; else the explicit branch L67-86): Y[i] = (internal, boundary) pairs (old time level), phiJmY[i], diffusiveFlux[i]
    per species (numpy arrays over the faces, updated in place), Su[i] explicit sources or None.  Returns the list of new cell fields:
    the active species from speciesStep, the inert one as 1 - sum of the others, clipped at 0 [L86-91]."""
    n = len(Y)
    new = [None] * n
    Yt = np.zeros(dev.mesh.nCells)                                # volScalarField Yt(0.0*Y[0])
    for i in range(n):
        if i != inertIndex and (active is None or active[i]):
            if implicitDiffusion:
                new[i], _ = speciesStepImplicit(dev, Y[i], rhoOld, rho, phiJmY[i], muf, ScNumbers[i], deltaT, diffusiveFlux[i], None if Su is None else Su[i],
                                                None if fixedValueFaces is None else fixedValueFaces[i], tolerance, maxIter, call)
            else:
                new[i] = speciesStep(dev, Y[i], rhoOld, rho, phiJmY[i], muf, ScNumbers[i], deltaT, diffusiveFlux[i], None if Su is None else Su[i], call)
            diffusiveFlux[inertIndex] -= diffusiveFlux[i]           # L65 / L83 (as listed: the running total of species i, not this step's increment)
            Yt += new[i]
    for i in range(n):
        if new[i] is None and i != inertIndex:
            new[i] = np.array(Y[i][0], dtype=float)                # inactive species keep their values
    new[inertIndex] = np.maximum(1.0 - Yt, 0.0)                    # L90-91
    return new
