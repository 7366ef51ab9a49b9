"""Run monitors of a resident QGDFoam case (qgd_monitor_* of include/qgd_amd.h) and the function objects of
``system/controlDict`` the QGDFoam application serves with them.

A ``Monitor`` is created once (``QGDFoamCase.monitor(probes=..., patches=...)``); ``sample()`` enqueues the pass and a small copy
on the case's stream and returns at once, ``read()`` waits for that sample only.  Four slots form a ring, so a loop can read a
sample a step or two after it was taken and never drain the stream.

With ``species=True`` on a case that carries species every sample holds the species block as well (qgd_monitor_enable_species):
``read()`` then also gives, per species in the case's order and with the inert one included, ``speciesMass`` [nS], ``speciesMin`` /
``speciesMinCell`` / ``speciesMax`` / ``speciesMaxCell`` [nS], ``speciesProbes`` [nProbes, nS], ``speciesPatchFlux`` [nPatches, nS], and
the scalars ``speciesFluxState``, ``speciesSumDefect``, ``speciesNonFinite``, ``speciesFirstNonFinite``.

A resident QHDFoam / SRFQHDFoam case has a ``QHDMonitor`` (``QHDFoamCase.monitor``; qgd_qhd_monitor_create) on the same slot ring: its
samples (``unpack_qhd``) carry the integrals of U, T, kinetic energy, p and of the body force, the continuity errors of the pressure solve,
the extrema of |U|, T, p and of the cells' continuity error, probes, and per patch the totals of phi and of the net face terms;
``QHDFunctionObjects`` serves the ``functions{}`` of the two applications from it.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _lib as L

INTEGRALS = ("volume", "mass", "momentum_x", "momentum_y", "momentum_z", "totalEnergy", "internalEnergy", "kineticEnergy")
EXTREMA_FIELDS = ("rho", "p", "T", "magU", "Mach")
PROBE_COLUMNS = ("rho", "Ux", "Uy", "Uz", "p", "T", "e")
PATCH_COLUMNS = ("area", "massFlux", "momentumFlux_x", "momentumFlux_y", "momentumFlux_z", "energyFlux",
                 "pressureForce_x", "pressureForce_y", "pressureForce_z")
# the result block of a QHD monitor (QHDMonitor, unpack_qhd)
QHD_INTEGRALS = ("volume", "U_x", "U_y", "U_z", "T", "kineticEnergy", "p", "bodyForce_x", "bodyForce_y", "bodyForce_z",
                 "continuityGlobal", "continuityLocal")
QHD_EXTREMA_FIELDS = ("magU", "T", "p", "contErr")
QHD_PROBE_COLUMNS = ("Ux", "Uy", "Uz", "T", "p")
QHD_PATCH_COLUMNS = ("area", "volumetricFlux", "UFlux_x", "UFlux_y", "UFlux_z", "TFlux",
                     "pressureForce_x", "pressureForce_y", "pressureForce_z")


class _MonitorBase:
    """what the monitors of either case kind share: the handle, the layout and the ring of four slots.  ``_create`` names the entry that
    makes the handle; qgd_monitor_layout / _sample / _read / _free serve both kinds."""
    _create = None

    def __init__(self, case, probes=None, patches=None):
        self.case = case
        self.probes = np.ascontiguousarray(probes if probes is not None else [], dtype=np.int32).reshape(-1)
        self.patches = np.ascontiguousarray(patches if patches is not None else [], dtype=np.int32).reshape(-1)
        spec = L.MonitorSpec()
        spec.nProbes, spec.nPatches = int(self.probes.size), int(self.patches.size)
        spec.probeCells = self.probes.ctypes.data_as(L.c_int32_p) if self.probes.size else None
        spec.patches = self.patches.ctypes.data_as(L.c_int32_p) if self.patches.size else None
        h = C.c_void_p()
        L.check(getattr(L.lib, self._create)(case._h, C.byref(spec), C.byref(h)), self._create)
        self._handle = L.NativeHandle(h, L.lib.qgd_monitor_free)
        off = (C.c_int64 * L.MONITOR_SECTIONS)()
        n, cap = C.c_int64(), C.c_int32()
        L.check(L.lib.qgd_monitor_layout(h, off, C.byref(n), C.byref(cap)), "qgd_monitor_layout")
        self.offsets, self.n_doubles, self.grid_cap = [int(x) for x in off], int(n.value), int(cap.value)
        self._pending = collections.deque()   # sampled and not yet read, oldest first
        self._last = -1

    @property
    def _h(self):
        return self._handle.value

    def sample(self, slot=None):
        """enqueue one sample on the case's stream (no host wait); slot None: the next slot of the ring.  Returns the slot."""
        if slot is None:
            slot = (self._last + 1) % L.MONITOR_SLOTS
        L.check(L.lib.qgd_monitor_sample(self._h, int(slot)), "qgd_monitor_sample")
        if slot in self._pending:          # sampled again before it was read: the older sample is gone
            self._pending.remove(slot)
        self._pending.append(slot)
        self._last = slot
        return slot

    def read_raw(self, slot=None):
        """(result block, time, step) of a slot; slot None: the oldest sample not read yet"""
        if slot is None:
            if not self._pending:
                raise ValueError("Monitor.read: no sample is waiting to be read")
            slot = self._pending[0]
        out = np.empty(self.n_doubles)
        t, step = C.c_double(), C.c_int64()
        L.check(L.lib.qgd_monitor_read(self._h, int(slot), out.ctypes.data_as(L.c_double_p), out.size, C.byref(t), C.byref(step)),
                "qgd_monitor_read")
        if slot in self._pending:
            self._pending.remove(slot)
        return out, t.value, int(step.value)

    def close(self):
        if getattr(self, "_handle", None):
            self._handle.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Monitor(_MonitorBase):
    _create = "qgd_monitor_create"

    def __init__(self, case, probes=None, patches=None, species=False):
        """probes: cell labels of the case's device mesh (-1: not on this rank, its row reads NaN); patches: patch indices; species: the
        samples carry the species block too (a case with set_species)"""
        super().__init__(case, probes, patches)
        h, off, n = self._h, (C.c_int64 * L.MONITOR_SECTIONS)(), C.c_int64()
        self.species, self.species_offsets, self.species_doubles = bool(species), None, 0
        if self.species:
            try:
                L.check(L.lib.qgd_monitor_enable_species(h), "qgd_monitor_enable_species")
                L.check(L.lib.qgd_monitor_species_layout(h, off, C.byref(n)), "qgd_monitor_species_layout")
            except Exception:
                self._handle.free()
                raise
            self.species_offsets, self.species_doubles = [int(x) for x in off], int(n.value)

    def read_species_raw(self, slot):
        """the species block of a slot (the sample qgd_monitor_read of that slot gives)"""
        out = np.empty(max(self.species_doubles, 1))[:self.species_doubles]
        L.check(L.lib.qgd_monitor_species_read(self._h, int(slot), out.ctypes.data_as(L.c_double_p), out.size), "qgd_monitor_species_read")
        return out

    def read(self, slot=None):
        if slot is None and self._pending:
            slot = self._pending[0]
        raw, t, step = self.read_raw(slot)
        s = unpack(raw, self.offsets, t, step)
        if self.species:
            s.update(unpack_species(self.read_species_raw(slot), self.species_offsets))
        return s


class QHDMonitor(_MonitorBase):
    """the run monitor of a resident QHDFoam / SRFQHDFoam case (``QHDFoamCase.monitor``; qgd_qhd_monitor_create): the same ring of four
    slots, the QHD result block (``unpack_qhd``)"""
    _create = "qgd_qhd_monitor_create"

    def read(self, slot=None):
        raw, t, step = self.read_raw(slot)
        return unpack_qhd(raw, self.offsets, t, step)


def _sections(raw, offsets, time, step, extrema_fields, probe_columns, patch_columns):
    """the five sections of a flow or QHD result block (header, integrals, extrema, probes, patches) and the keys both blocks name alike"""
    o = offsets
    hd, integ = raw[o[0]:o[1]], raw[o[1]:o[2]]
    ex = raw[o[2]:o[3]].reshape(len(extrema_fields), 4)
    n_probes, n_patches = int(hd[2]), int(hd[3])
    probes = raw[o[3]:o[4]].reshape(n_probes, len(probe_columns))
    patches = raw[o[4]:o[4] + n_patches * len(patch_columns)].reshape(n_patches, len(patch_columns))
    return hd, integ, dict(time=time, step=step, deltaT=float(hd[6]), ownedCells=int(hd[0]), fluxState=int(hd[1]),
                           nonFinite=int(hd[4]), firstNonFinite=int(hd[5]), integrals=integ.copy(),
                           min=ex[:, 0].copy(), minCell=ex[:, 1].astype(np.int64), max=ex[:, 2].copy(), maxCell=ex[:, 3].astype(np.int64),
                           probes=probes.copy(), patchArea=patches[:, 0].copy(), patchFlux=patches[:, 1:6].copy(),
                           patchPressureForce=patches[:, 6:9].copy(), raw=raw)


# the keys a sample derives from its integrals: a scalar by its index, a vector by its slice (unpack, unpack_qhd and combine)
_FLOW_DERIVED = dict(volume=0, mass=1, momentum=slice(2, 5), totalEnergy=5, internalEnergy=6, kineticEnergy=7)
_QHD_DERIVED = dict(volume=0, momentum=slice(1, 4), bodyForce=slice(7, 10), continuityGlobal=10, continuityLocal=11)


def _derived(integ, table):
    return {key: integ[at].copy() if isinstance(at, slice) else float(integ[at]) for key, at in table.items()}


def unpack(raw, offsets, time, step):
    """named arrays of one result block (the layout of include/qgd_amd.h)"""
    # fluxState 0: no assembly yet (patch fluxes NaN); 1: all five; 2: implicitDiffusion (mass flux only, the other four NaN)
    hd, integ, s = _sections(raw, offsets, time, step, EXTREMA_FIELDS, PROBE_COLUMNS, PATCH_COLUMNS)
    s.update(_derived(integ, _FLOW_DERIVED))
    return s


def unpack_qhd(raw, offsets, time, step):
    """named arrays of one result block of a QHD monitor (the layout of include/qgd_amd.h, qgd_qhd_monitor_create); the keys are those of
    ``unpack`` wherever the meaning is the same"""
    # fluxState 0: no step yet (patch fluxes and continuity entries NaN); 1: everything; 2: implicitDiffusion (the U / T flux columns NaN)
    hd, integ, s = _sections(raw, offsets, time, step, QHD_EXTREMA_FIELDS, QHD_PROBE_COLUMNS, QHD_PATCH_COLUMNS)
    flags = int(hd[7])
    s.update(_derived(integ, _QHD_DERIVED), kind="qhd", rotating=bool(flags & 1), frozenT=bool(flags & 2))
    return s


def unpack_species(raw, offsets):
    """named arrays of one species block (the layout of include/qgd_amd.h, qgd_monitor_enable_species); all species, the inert one included"""
    o = offsets
    hd = raw[o[0]:o[1]]
    n_s, n_probes, n_patches = int(hd[0]), int(hd[6]), int(hd[7])
    ex = raw[o[2]:o[3]].reshape(n_s, 4)
    # speciesFluxState 0: no species assembly since set_fields (speciesPatchFlux NaN); 1: explicit branch; 2: implicitDiffusion
    return dict(nSpecies=n_s, speciesInert=int(hd[1]), speciesFluxState=int(hd[2]), speciesNonFinite=int(hd[3]), speciesFirstNonFinite=int(hd[4]),
                speciesSumDefect=float(hd[5]), speciesMass=raw[o[1]:o[2]].copy(),
                speciesMin=ex[:, 0].copy(), speciesMinCell=ex[:, 1].astype(np.int64), speciesMax=ex[:, 2].copy(), speciesMaxCell=ex[:, 3].astype(np.int64),
                speciesProbes=raw[o[3]:o[4]].reshape(n_probes, n_s).copy(),
                speciesPatchFlux=raw[o[4]:o[4] + n_patches * n_s].reshape(n_patches, n_s).copy(), speciesRaw=raw)


_FLOW_KEYS = dict(sums=("integrals", "momentum", "patchArea", "patchFlux", "patchPressureForce"), count="nonFinite", first="firstNonFinite",
                  extrema=(("min", "minCell", 1.0), ("max", "maxCell", -1.0)), probes="probes")
_SPECIES_KEYS = dict(sums=("speciesMass", "speciesPatchFlux"), count="speciesNonFinite", first="speciesFirstNonFinite",
                     extrema=(("speciesMin", "speciesMinCell", 1.0), ("speciesMax", "speciesMaxCell", -1.0)), probes="speciesProbes")


def combine(parts):
    """the samples of the ranks of one run as one: sums in rank order, extrema by (value, label) with ties to the lowest label, a probe
    from the rank that holds its cell (the others carry NaN rows), patch totals summed.  The species block of the parts (Monitor with
    species=True) is merged the same way; speciesSumDefect is the largest of the ranks'.  (Nothing here has run on more than one GPU: the
    parts of the tests are shards on one device.)"""
    out = dict(parts[0])
    if len(parts) == 1:
        return out
    _combine_block(out, parts, _FLOW_KEYS)
    # the derived keys of the kind; the flags and the flux state of a QHD sample are the same on every shard
    out.update(_derived(out["integrals"], _QHD_DERIVED if parts[0].get("kind") == "qhd" else _FLOW_DERIVED),
               ownedCells=sum(p["ownedCells"] for p in parts))
    if "speciesMass" in parts[0]:
        _combine_block(out, parts, _SPECIES_KEYS)
        defects = [p["speciesSumDefect"] for p in parts if not np.isnan(p["speciesSumDefect"])]
        out["speciesSumDefect"] = max(defects) if defects else float("nan")
        out.pop("speciesRaw", None)
    out.pop("raw", None)
    return out


def _combine_block(out, parts, keys):
    for key in keys["sums"]:
        acc = np.array(parts[0][key], dtype=np.float64)
        for p in parts[1:]:
            acc = acc + p[key]
        out[key] = acc
    out[keys["count"]] = sum(p[keys["count"]] for p in parts)
    bad = [p[keys["first"]] for p in parts if p[keys["first"]] >= 0]
    out[keys["first"]] = min(bad) if bad else -1
    for val, cell, sign in keys["extrema"]:
        v, c = np.array(parts[0][val]), np.array(parts[0][cell])
        for p in parts[1:]:
            for k in range(v.size):
                if p[cell][k] < 0:
                    continue
                better = c[k] < 0 or sign * p[val][k] < sign * v[k] or (p[val][k] == v[k] and p[cell][k] < c[k])
                if better:
                    v[k], c[k] = p[val][k], p[cell][k]
        out[val], out[cell] = v, c
    probes = np.array(parts[0][keys["probes"]])
    for p in parts[1:]:
        take = np.isnan(probes).all(axis=1) & ~np.isnan(p[keys["probes"]]).all(axis=1)
        probes[take] = p[keys["probes"]][take]
    out[keys["probes"]] = probes


# ---- the function objects of system/controlDict (foamfile.read_functions gives the specifications) ----------------------------------------
def _num(x):
    return f"{float(x):.17g}"


class _Table:
    """one output file: header once, one row per write"""

    def __init__(self, path, header_lines):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        self.path = path
        with open(path, "w") as f:
            f.write("".join(line + "\n" for line in header_lines))

    def row(self, text):
        with open(self.path, "a") as f:
            f.write(text + "\n")


class ProbesWriter:
    """OpenFOAM's probes layout: postProcessing/<name>/<startTime>/<field>, one file per field, `# Probe i (x y z)` lines, the probe
    numbers, `# Time`, then one row per write: the time and one value per probe (vectors in parentheses)"""
    _COLS = {"rho": (0,), "U": (1, 2, 3), "p": (4,), "T": (5,), "e": (6,)}

    def __init__(self, out_dir, spec, found, species=()):
        self.fields = list(spec["fields"])
        self.species = list(species)          # the case's species names: a field among them is a column of speciesProbes
        locs = np.asarray(spec["probeLocations"], dtype=np.float64).reshape(-1, 3)
        head = [f"# Probe {i} ({_num(x[0])} {_num(x[1])} {_num(x[2])})" + ("" if found[i] else "  # Not Found") for i, x in enumerate(locs)]
        head.append("# Probe " + " ".join(str(i) for i in range(len(locs))))
        head.append("# Time")
        self.tables = {f: _Table(os.path.join(out_dir, f), head) for f in self.fields}

    def write(self, t, s):
        for f, table in self.tables.items():
            if f not in self._COLS:
                k = self.species.index(f)
                table.row(" ".join([_num(t)] + [_num(r[k]) for r in s["speciesProbes"]]))
                continue
            cols = self._COLS[f]
            vals = [(_num(r[cols[0]]) if len(cols) == 1 else "(" + " ".join(_num(r[c]) for c in cols) + ")") for r in s["probes"]]
            table.row(" ".join([_num(t)] + vals))


class FieldMinMaxWriter:
    """fieldMinMax.dat: per write one row -- the time, then per field min, its cell and the cell's centre, max, its cell and centre
    (U stands for mag(U), as fieldMinMax's default mode has it)"""
    _INDEX = {"rho": 0, "p": 1, "T": 2, "U": 3, "mag(U)": 3, "Mach": 4}

    def __init__(self, out_dir, spec, centres, file_label, species=()):
        self.fields = list(spec["fields"])
        self.species = list(species)          # the case's species names: a field among them reads speciesMin / speciesMax
        self.centres, self.file_label = centres, file_label
        cols = ["Time"]
        for f in self.fields:
            n = "mag(U)" if f == "U" else f
            for w in ("min", "max"):
                cols += [f"{w}({n})", f"cell({w})", f"x({w})", f"y({w})", f"z({w})"]
        self.table = _Table(os.path.join(out_dir, "fieldMinMax.dat"), ["# Field minima and maxima", "# " + "\t".join(cols)])

    def write(self, t, s):
        row = [_num(t)]
        for f in self.fields:
            if f in self._INDEX:
                k, keys = self._INDEX[f], (("min", "minCell"), ("max", "maxCell"))
            else:
                k, keys = self.species.index(f), (("speciesMin", "speciesMinCell"), ("speciesMax", "speciesMaxCell"))
            for val, cell in keys:
                c = int(s[cell][k])
                x = self.centres[c] if c >= 0 else (np.nan,) * 3
                row += [_num(s[val][k]), str(int(self.file_label[c]) if c >= 0 else -1)] + [_num(v) for v in x]
        self.table.row("\t".join(row))


class IntegralsWriter:
    """volIntegrals.dat: the time, the volume integrals of the block (``COLUMNS``: the eight of a QGDFoam case), the count of non-finite
    cells and the first of them (-1: none)"""
    COLUMNS = INTEGRALS

    def __init__(self, out_dir, spec, file_label):
        self.file_label = file_label
        self.table = _Table(os.path.join(out_dir, "volIntegrals.dat"),
                            ["# Volume integrals over the mesh", "# " + "\t".join(("Time",) + self.COLUMNS + ("nonFiniteCells", "firstNonFiniteCell"))])

    def write(self, t, s):
        first = int(self.file_label[s["firstNonFinite"]]) if s["firstNonFinite"] >= 0 else -1
        self.table.row("\t".join([_num(t)] + [_num(v) for v in s["integrals"]] + [str(int(s["nonFinite"])), str(first)]))


class PatchFluxWriter:
    """patchFluxes.dat: the time, then per patch the columns of the block's patch row (``COLUMNS``) -- for a QGDFoam case its area, the
    five net fluxes out of the domain (mass, momentum, total energy: what the cell update consumed in the step that produced the state)
    and sum p_b Sf"""
    COLUMNS, TITLE = PATCH_COLUMNS, "# Patch totals of the net face fluxes"

    def __init__(self, out_dir, spec, rows):
        self.rows = rows                    # rows of the monitor's patch table, in the order of spec["patches"]
        cols = ["Time"] + [f"{p}:{c}" for p in spec["patches"] for c in self.COLUMNS]
        self.table = _Table(os.path.join(out_dir, "patchFluxes.dat"), [self.TITLE, "# " + "\t".join(cols)])

    def write(self, t, s):
        row = [_num(t)]
        for r in self.rows:
            row += [_num(s["patchArea"][r])] + [_num(v) for v in s["patchFlux"][r]] + [_num(v) for v in s["patchPressureForce"][r]]
        self.table.row("\t".join(row))


class SpeciesIntegralsWriter:
    """speciesIntegrals.dat: the time, sum rho Y_i V per species (the inert one included), max |sum_i Y_i - 1|, the count of cells with a
    non-finite Y_i and the first of them (-1: none)"""

    def __init__(self, out_dir, spec, file_label, species):
        self.file_label = file_label
        cols = ["Time"] + [f"mass({n})" for n in species] + ["sumDefect", "nonFiniteCells", "firstNonFiniteCell"]
        self.table = _Table(os.path.join(out_dir, "speciesIntegrals.dat"), ["# Species masses over the mesh", "# " + "\t".join(cols)])

    def write(self, t, s):
        first = int(self.file_label[s["speciesFirstNonFinite"]]) if s["speciesFirstNonFinite"] >= 0 else -1
        self.table.row("\t".join([_num(t)] + [_num(v) for v in s["speciesMass"]] + [_num(s["speciesSumDefect"]), str(int(s["speciesNonFinite"])), str(first)]))


class SpeciesPatchFluxWriter:
    """speciesPatchFluxes.dat: the time, then per patch the net flux of every species out of the domain (what the species' cell update
    consumed in the step that produced the state; the inert species: the mass flux minus the others')"""

    def __init__(self, out_dir, spec, rows, species):
        self.rows = rows                    # rows of the monitor's patch table, in the order of spec["patches"]
        cols = ["Time"] + [f"{p}:{n}" for p in spec["patches"] for n in species]
        self.table = _Table(os.path.join(out_dir, "speciesPatchFluxes.dat"), ["# Patch totals of the net species fluxes", "# " + "\t".join(cols)])

    def write(self, t, s):
        row = [_num(t)]
        for r in self.rows:
            row += [_num(v) for v in s["speciesPatchFlux"][r]]
        self.table.row("\t".join(row))


SPECIES_TYPES = ("qgdSpeciesIntegrals", "qgdSpeciesPatchFluxes")


class FunctionObjects:
    """the served functions of a run: one Monitor for all of them, sampled after the steps at which a function is due, read two samples
    late.  ``local_of`` maps a cell label of the file mesh (as relabelled for the device) to this rank's label or -1; ``file_label`` maps
    it back to the label in the case files; ``gather`` (None on one rank) is all_gather_object.  ``species``: the case's species names;
    a function that names one of them, or one of SPECIES_TYPES, makes the monitor carry the species block."""

    _PROBES, _MINMAX = ProbesWriter, FieldMinMaxWriter      # the writers of the two types every application serves

    def _open_monitor(self, case, probes, patches, species):
        return Monitor(case, probes=probes, patches=patches, species=species)

    def _own_writer(self, s, out_dir, file_label, patch_rows, species):
        """the writer of one of the application's own types (root only)"""
        if s["type"] == "qgdIntegrals":
            return IntegralsWriter(out_dir, s, file_label)
        if s["type"] == "qgdPatchFluxes":
            return PatchFluxWriter(out_dir, s, [patch_rows[p] for p in s["patches"]])
        if s["type"] == "qgdSpeciesIntegrals":
            return SpeciesIntegralsWriter(out_dir, s, file_label, species)
        if s["type"] == "qgdSpeciesPatchFluxes":
            return SpeciesPatchFluxWriter(out_dir, s, [patch_rows[p] for p in s["patches"]], species)
        return None

    def __init__(self, case, specs, file_mesh, case_dir, start_name, local_of, file_label, is_root=True, gather=None, log=print, species=None):
        self.specs, self.is_root, self.gather = specs, is_root, gather
        species = list(species or [])
        flow_fields = set(self._PROBES._COLS) | set(self._MINMAX._INDEX)
        wanted = [(s["name"], f) for s in specs for f in s.get("fields", []) if f not in flow_fields] + [(s["name"], s["type"]) for s in specs if s["type"] in SPECIES_TYPES]
        for name, what in wanted:
            if what not in species and what not in SPECIES_TYPES:
                raise ValueError(f"functions: '{name}': field '{what}' is neither a flow field nor a species of this case (species: {', '.join(species) or 'none'})")
            if not species:
                raise ValueError(f"functions: '{name}': type {what} needs a case with species; this case carries none")
        locations = [np.asarray(s["probeLocations"], dtype=np.float64).reshape(-1, 3) for s in specs if s["type"] == "probes"]
        cells = file_mesh.find_cells(np.concatenate(locations)) if locations else np.zeros(0, dtype=np.int64)
        names = list(getattr(file_mesh, "patch_names", []))
        patch_rows, patches = {}, []
        for s in specs:
            for p in s.get("patches", []):
                if p not in names:
                    raise ValueError(f"functions: '{s['name']}': no patch named '{p}' (patches: {', '.join(names)})")
                if p not in patch_rows:
                    patch_rows[p] = len(patches)
                    patches.append(names.index(p))
        self.monitor = self._open_monitor(case, [local_of(int(c)) if c >= 0 else -1 for c in cells], patches, bool(wanted))
        self.writers = []
        centres = file_mesh.array("C").reshape(-1, 3)
        at = 0
        for s in specs:
            out_dir = os.path.join(case_dir, "postProcessing", s["name"], start_name)
            w = None
            if s["type"] == "probes":
                n = len(np.asarray(s["probeLocations"]).reshape(-1, 3))
                rows = slice(at, at + n)
                at += n
                if is_root:
                    for i, c in enumerate(cells[rows]):
                        if c < 0:
                            log(f"functions: '{s['name']}': probe {i} is outside the mesh: its column reads nan")
                    w = self._PROBES(out_dir, s, cells[rows] >= 0, species)
                    w.rows = rows
            elif not is_root:
                pass
            elif s["type"] == "fieldMinMax":
                w = self._MINMAX(out_dir, s, centres, file_label, species)
            else:
                w = self._own_writer(s, out_dir, file_label, patch_rows, species)
            self.writers.append(w)
        self._waiting = collections.deque()   # (due specs) of the samples not read yet

    def next_due(self, step):
        """steps from `step` to the next one at which some function writes"""
        return min(s["interval"] - step % s["interval"] for s in self.specs)

    def after_step(self, step, t0):
        due = [i for i, s in enumerate(self.specs) if step % s["interval"] == 0]
        if not due:
            return
        self.monitor.sample()
        self._waiting.append((due, t0))
        while len(self._waiting) > 2:
            self._flush_one()

    def _flush_one(self):
        due, t0 = self._waiting.popleft()
        s = self.monitor.read()
        if self.gather is not None:
            s.pop("raw", None)
            s.pop("speciesRaw", None)
            s = combine(self.gather(s))
        if not self.is_root:
            return
        t = t0 + s["time"]
        for i in due:
            w = self.writers[i]
            if isinstance(w, ProbesWriter):
                w.write(t, dict(s, probes=s["probes"][w.rows], **({"speciesProbes": s["speciesProbes"][w.rows]} if "speciesProbes" in s else {})))
            elif w is not None:
                w.write(t, s)

    def finish(self):
        while self._waiting:
            self._flush_one()
        self.monitor.close()


# ---- the function objects of a QHDFoam / SRFQHDFoam case (foamfile.read_qhd_functions gives the specifications) ---------------------------
class QHDProbesWriter(ProbesWriter):
    """the probes layout on the probe rows of a QHD sample"""
    _COLS = {"U": (0, 1, 2), "T": (3,), "p": (4,)}


class QHDFieldMinMaxWriter(FieldMinMaxWriter):
    """fieldMinMax.dat on the extrema of a QHD sample; contErr is |sum of phi over the cell's faces| / V"""
    _INDEX = {"U": 0, "mag(U)": 0, "T": 1, "p": 2, "contErr": 3}


class QHDIntegralsWriter(IntegralsWriter):
    """volIntegrals.dat with the twelve integrals of the QHD block"""
    COLUMNS = QHD_INTEGRALS


class QHDPatchFluxWriter(PatchFluxWriter):
    """patchFluxes.dat of a QHD sample: per patch its area, the volumetric flux, the totals of the net face terms of the U (3) and T
    equations (what the cell update consumed in the step that produced the state) and sum p_b Sf"""
    COLUMNS, TITLE = QHD_PATCH_COLUMNS, "# Patch totals of phi and of the net face terms"


class ContinuityErrorsWriter:
    """continuityErrors.dat, what OpenFOAM's continuityErrs.H prints: the time, sum local = deltaT sum |d_c| / sum V, global =
    deltaT sum d_c / sum V, the cumulative global error over the rows written, and the largest |d_c| / V_c with its cell
    (d_c: the signed sum of phi over the faces of cell c)"""

    def __init__(self, out_dir, spec, file_label):
        self.file_label, self.cumulative = file_label, 0.0
        cols = ("Time", "sumLocal", "global", "cumulative", "max(contErr)", "cell(max)")
        self.table = _Table(os.path.join(out_dir, "continuityErrors.dat"), ["# Continuity errors of the pressure solve", "# " + "\t".join(cols)])

    def write(self, t, s):
        local, glob = continuity_errors(s)
        self.cumulative += glob
        c = int(s["maxCell"][3])
        self.table.row("\t".join([_num(t), _num(local), _num(glob), _num(self.cumulative), _num(s["max"][3]), str(int(self.file_label[c]) if c >= 0 else -1)]))


def continuity_errors(s):
    """(sum local, global) continuity errors of a QHD sample, as OpenFOAM scales them"""
    scale = s["deltaT"] / s["volume"]
    return scale * s["continuityLocal"], scale * s["continuityGlobal"]


class QHDFunctionObjects(FunctionObjects):
    """FunctionObjects for a QHDFoam or SRFQHDFoam run: one QHDMonitor, the QHD writers"""
    _PROBES, _MINMAX = QHDProbesWriter, QHDFieldMinMaxWriter

    def _open_monitor(self, case, probes, patches, species):
        return QHDMonitor(case, probes=probes, patches=patches)

    def _own_writer(self, s, out_dir, file_label, patch_rows, species):
        if s["type"] == "qhdIntegrals":
            return QHDIntegralsWriter(out_dir, s, file_label)
        if s["type"] == "qhdPatchFluxes":
            return QHDPatchFluxWriter(out_dir, s, [patch_rows[p] for p in s["patches"]])
        if s["type"] == "qhdContinuityErrors":
            return ContinuityErrorsWriter(out_dir, s, file_label)
        return None
