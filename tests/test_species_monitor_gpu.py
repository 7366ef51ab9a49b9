"""The species block of a run monitor (qgd_monitor_enable_species, qgdsolver_amd/csrc/qgd_monitor_species.hip): masses, extrema, probes
and patch totals of every species against numpy on the case's own fields, the discrete species balance they close on either branch,
ghosts, non-interference, refusals and the application.

Sums are compared with math.fsum of their terms under the bound n * 2^-52 * sum |term| (n terms), which holds for every order of
summation; extrema, their labels, probe values and the sum defect exactly (Y_i is a stored field, the defect is summed in species
order on both sides)."""
import math
import os

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd import foamfile as ff
from qgdsolver_amd.monitor import combine
import cases
from test_monitor_gpu import EPS, io_bcs, sum_ok
from test_species_reader import SPECIES, write_species_case
from util import assert_path, make_mesh

pytestmark = pytest.mark.gpu

G, E = L.PATCH_GENERIC, L.PATCH_EMPTY
DIMS = {"box111": (1, 1, 1), "box5_3_17": (5, 3, 17), "box488": (4, 8, 8), "box257_1_1": (257, 1, 1), "box64_64_65": (64, 64, 65),
        "box128_128_65": (128, 128, 65)}


def mesh_of(kind):
    return q.PolyMesh.box(*DIMS[kind]) if kind in DIMS else make_mesh(kind)


def composition(C, nS, inert):
    """nS species: the transported ones within 0.5 / (nS - 1) * [0.6, 1.4], their sum and the inert one within [0.3, 0.7]"""
    amp = 0.5 / (nS - 1)
    Y = [amp * (1.0 + 0.4 * np.sin((1.0 + 0.5 * i) * np.pi * C[:, 0] + 0.7 * i) * np.cos((0.5 + 0.3 * i) * np.pi * C[:, 1])) for i in range(nS - 1)]
    Y.insert(inert, 1.0 - sum(Y))
    return Y


def schmidt(nS):
    return [0.7 + 0.6 * ((3 * i) % 7) / 7.0 for i in range(nS)]


def species_case(mesh, nS, inert, bc_fn=None, species_bcs=(), Y0=None, fields=None, cells=None, implicit=False, keep=False, halo=False, **opt):
    """a case on the separate kernels with nS species; species_bcs: (species, patch, entry); cells: the labels of the uncut mesh of a
    shard's cells (fields and Y0 are then those of the uncut mesh)"""
    opt = dict(dict(stencil="GaussVolPoint" if mesh.nGeometricD == 3 else "leastSquares", deltaT=1e-3, mu=1e-3), **opt)
    if implicit:
        opt = dict(dict(implicitDiffusion=1, implicitTol=1e-14, implicitMaxIter=2000), **opt)
    dev = q.Device(mesh, fused_tables=False)
    case = q.QGDFoamCase(dev, q.default_options(**opt))
    if bc_fn:
        bc_fn(case)
    names = [f"S{i}" for i in range(nS)]
    case.set_species(names, inert, ScNumbers=schmidt(nS), keep_fluxes=keep, implicit=implicit, halo=halo)
    for i, patch, entry in species_bcs:
        case.set_species_bc(i, patch, entry)
    C = mesh.array("C").reshape(-1, 3)
    if Y0 is None:
        Y0 = composition(C, nS, inert)
    for i in range(nS):
        case.set_species_field(i, Y0[i] if cells is None else Y0[i][cells])
    U, T, p = fields if fields is not None else cases.box_initial_fields(C)
    if cells is not None:
        U, T, p = U[cells], T[cells], p[cells]
    case.set_fields(U, T, p)
    assert_path(case, "kernels")
    return dev, case


def check_species_cells(s, case, V, nS, owned=None, labels=None, what=""):
    owned = np.arange(V.size) if owned is None else owned
    labels = owned if labels is None else labels
    rho = case.field("rho")[owned]
    V = V[owned]
    Y = [case.species_field(i)[owned] for i in range(nS)]
    assert s["nSpecies"] == nS and s["speciesNonFinite"] == 0 and s["speciesFirstNonFinite"] == -1
    ysum = np.zeros(owned.size)
    for i in range(nS):
        ysum = ysum + Y[i]
        sum_ok(s["speciesMass"][i], rho * Y[i] * V, f"{what} mass of species {i}")
        for val, cell, arg in (("speciesMin", "speciesMinCell", np.argmin), ("speciesMax", "speciesMaxCell", np.argmax)):
            k = int(arg(Y[i]))                    # numpy's first occurrence: the lowest label of a tie
            assert s[val][i] == Y[i][k] and s[cell][i] == labels[k], (what, val, i, s[val][i], Y[i][k], s[cell][i], labels[k])
    defect = float(np.abs(ysum - 1.0).max())
    print(f"{what} sum defect: got {s['speciesSumDefect']!r} numpy {defect!r}")
    assert s["speciesSumDefect"] == defect


def check_species_probes(s, case, cells, nS):
    Y = [case.species_field(i) for i in range(nS)]
    assert s["speciesProbes"].shape == (len(cells), nS)
    for row, c in zip(s["speciesProbes"], cells):
        if c < 0:
            assert np.isnan(row).all()
        else:
            assert np.array_equal(row, [Y[i][c] for i in range(nS)])


# ---- 1. integrals, extrema and probes against numpy -----------------------------------------------------------------------------------------
CELL_CASES = [(k, 6) for k in ("box111", "box5_3_17", "box257_1_1", "box488", "box654_poly", "box64_64_65")]
CELL_CASES += [("box5_3_17", 2), ("box654_poly", 2), ("box5_3_17", 5), ("box654_poly", 5), ("box5_3_17", 32), ("box128_128_65", 2), ("tet433", 6), ("mix643", 5)]


@pytest.mark.parametrize("kind,nS", CELL_CASES)
def test_masses_extrema_and_probes_against_numpy(kind, nS):
    mesh = mesh_of(kind)
    assert {"box5_3_17": 255, "box488": 256, "box257_1_1": 257}.get(kind, mesh.nCells) == mesh.nCells
    assert nS <= L.MAX_SPECIES
    inert = nS // 2
    dev, case = species_case(mesh, nS, inert)
    assert case.species_info()["batchWidth"] == 4      # 2: one species in a batch; 5: a full batch and one; 6: a second, partial batch
    probes = sorted({0, mesh.nCells // 2, mesh.nCells - 1}) + [-1]
    m = case.monitor(probes=probes, species=True)
    assert m.species_offsets == [0, 8, 8 + nS, 8 + 5 * nS, 8 + 5 * nS + nS * len(probes)] and m.species_doubles == m.species_offsets[4]
    if kind == "box64_64_65":
        assert mesh.nCells > 256 * 1024                # tiles of 1024 cells: more partial rows than the fold has threads
    if kind == "box128_128_65":
        assert mesh.nCells > m.grid_cap * 1024         # more tiles than workgroups: a workgroup takes a second tile
    case.step(2)
    m.sample()
    s = m.read()
    assert s["step"] == 2 and s["speciesInert"] == inert and s["speciesFluxState"] == 1
    check_species_cells(s, case, mesh.array("V"), nS, what=f"{kind} nS {nS}")
    check_species_probes(s, case, probes, nS)
    case.close(); dev.close()


# ---- 2. ties and non-finite cells ---------------------------------------------------------------------------------------------------------
def test_uniform_composition_puts_every_extremum_at_the_first_owned_cell():
    mesh = q.PolyMesh.box(9, 8, 7)
    n, nS = mesh.nCells, 5
    uniform = lambda k: [np.full(k, 0.125)] * 2 + [np.full(k, 0.5)] + [np.full(k, 0.125)] * 2     # noqa: E731
    dev, case = species_case(mesh, nS, 2, Y0=uniform(n))
    m = case.monitor(species=True)
    m.sample()
    s = m.read()
    assert np.array_equal(s["speciesMinCell"], np.zeros(nS)) and np.array_equal(s["speciesMaxCell"], np.zeros(nS))
    assert np.array_equal(s["speciesMin"], s["speciesMax"]) and s["speciesMin"][2] == 0.5 and s["speciesSumDefect"] == 0.0
    case.close(); dev.close()
    # a shard: the first owned cell is not local cell 0, and its label is that of the unsharded mesh
    sh = mesh.shard(3, 1)
    cg = sh.array("cellGlobal")
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    dev, case = species_case(sh, nS, 2, Y0=uniform(n), fields=(U, T, p), cells=cg, halo=True)
    m = case.monitor(species=True)
    m.sample()
    s = m.read()
    first = n // 3
    assert first in cg and cg[0] < first
    assert np.array_equal(s["speciesMinCell"], np.full(nS, first)) and np.array_equal(s["speciesMaxCell"], np.full(nS, first))
    case.close(); dev.close()


def test_one_nan_in_one_species_is_counted_named_and_kept_out_of_that_species_only():
    mesh = q.PolyMesh.box(7, 6, 5)
    nS, bad, sick = 6, 137, 4
    Y0 = [y.copy() for y in composition(mesh.array("C").reshape(-1, 3), nS, 2)]
    Y0[sick][bad] = np.nan
    Y0[0][bad] = 0.75            # the largest value of species 0 sits in that very cell: it stays in species 0's extrema
    dev, case = species_case(mesh, nS, 2, Y0=Y0)
    m = case.monitor(species=True)
    m.sample()                   # no step taken
    s = m.read()
    assert s["speciesNonFinite"] == 1 and s["speciesFirstNonFinite"] == bad and s["nonFinite"] == 0
    assert s["speciesMax"][0] == 0.75 and s["speciesMaxCell"][0] == bad
    others = np.delete(np.arange(mesh.nCells), bad)
    y = Y0[sick][others]
    assert s["speciesMin"][sick] == y.min() and s["speciesMinCell"][sick] == others[np.argmin(y)]
    assert s["speciesMax"][sick] == y.max() and s["speciesMaxCell"][sick] == others[np.argmax(y)]
    for i in range(nS):
        if i != sick:
            assert s["speciesMin"][i] == Y0[i].min() and s["speciesMinCell"][i] == np.argmin(Y0[i])
            assert s["speciesMax"][i] == Y0[i].max() and s["speciesMaxCell"][i] == np.argmax(Y0[i])
            assert np.isfinite(s["speciesMass"][i])
    assert np.isnan(s["speciesMass"][sick])
    ysum = np.zeros(others.size)
    for i in range(nS):
        ysum = ysum + Y0[i][others]
    assert s["speciesSumDefect"] == np.abs(ysum - 1.0).max()      # over the cells whose Y_i are all finite
    case.close(); dev.close()


# ---- 3. patch totals against the kept face fields --------------------------------------------------------------------------------------------
def consumed_terms(case, mesh, i, inert, nS, phiJm, Yb_old, implicit, faces):
    """per face of `faces` the terms whose sum is the net flux of species i the species' cell update consumed, from the fields a case
    with QGD_SPECIES_KEEP_FLUXES keeps (by face label) -- rows of a 2-D array, one row per term.
    With dydt = phiJmY_i - phiJm Y_b (the QGD part of phiJmY_i; Y_b the patch value the step read) the headers give
      explicit branch (qgd_species.hip):           phiJmY_i - lap_i,   diffusiveFlux_i = dydt + lap_i   ->  phiJmY - diffusiveFlux + phiJmY - phiJm Y_b
      implicit branch (qgd_species_implicit.hip):  phiJmY_i + YEqn.flux(),   diffusiveFlux_i = dydt + YEqn.flux()   ->  phiJmY + diffusiveFlux - phiJmY + phiJm Y_b
    and for the inert species phiJm minus the others'."""
    nif = mesh.nInternalFaces
    if i == inert:
        rows = [phiJm[faces]]
        for a in range(nS):
            if a != inert:
                rows += list(-consumed_terms(case, mesh, a, inert, nS, phiJm, Yb_old, implicit, faces))
        return np.array(rows)
    pjy, df = case.species_field(i, "phiJmY")[faces], case.species_field(i, "diffusiveFlux")[faces]
    adv = phiJm[faces] * Yb_old[i][faces - nif]
    return np.array([pjy, df, -pjy, adv] if implicit else [pjy, -df, pjy, -adv])


def check_species_patches(s, case, mesh, patches, nS, inert, phiJm, Yb_old, implicit, faces_of=None, what=""):
    ps, pz = mesh.array("patchStart"), mesh.array("patchSize")
    for row, pa in enumerate(patches):
        f = np.arange(ps[pa], ps[pa] + pz[pa]) if faces_of is None else faces_of(pa)
        for i in range(nS):
            sum_ok(s["speciesPatchFlux"][row, i], consumed_terms(case, mesh, i, inert, nS, phiJm, Yb_old, implicit, f), f"{what} patch {pa} species {i}")


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("kind", ["box654_poly", "plane2d_jitter", "box257_257_1", "tet433"])
def test_patch_totals_against_the_kept_face_fields(kind, implicit):
    mesh = q.PolyMesh.box(257, 257, 1) if kind == "box257_257_1" else make_mesh(kind)
    if kind == "box257_257_1":
        assert list(mesh.array("patchSize")[4:6]) == [66049] * 2     # 259 chunks: the fold's threads take a second trip over a patch's rows
    nS, inert = 6, 2
    # species 0: fixedValue at the inlet, zero-gradient at the outlet; species 3: the other way round; species 5: fixedValue on a wall
    sbcs = [(0, 0, ("fixedValue", 0.3)), (3, 1, ("fixedValue", 0.05)), (5, 2, ("fixedValue", 0.2)), (1, 0, ("fixedValue", 0.1))]
    dev, case = species_case(mesh, nS, inert, bc_fn=io_bcs, species_bcs=sbcs, implicit=implicit, keep=True)
    if kind == "plane2d_jitter":
        with pytest.raises(q.QgdError, match="empty patch"):
            case.monitor(patches=[0, 4], species=True)
        patches = [3, 0, 1, 2, 0]
    else:
        patches = [5, 0, 1, 2, 3, 4, 0]                  # any order, one of them twice
    m = case.monitor(patches=patches, species=True)
    case.updateFluxes()
    phiJm = case.field("phiJm")
    Yb_old = [case.species_field(i, "Y.boundary") for i in range(nS)]
    case.step(1)
    m.sample()
    s = m.read()
    assert s["speciesFluxState"] == (2 if implicit else 1) and s["fluxState"] == (2 if implicit else 1)
    check_species_patches(s, case, mesh, patches, nS, inert, phiJm, Yb_old, implicit, what=f"{kind} implicit {implicit}")
    assert np.array_equal(s["speciesPatchFlux"][1], s["speciesPatchFlux"][-1])
    if implicit:    # the diffusive part is there: on its fixedValue patch a species' total is not that of phiJmY alone
        f = np.arange(mesh.array("patchStart")[0], mesh.array("patchStart")[0] + mesh.array("patchSize")[0])
        assert abs(s["speciesPatchFlux"][1, 0] - math.fsum(case.species_field(0, "phiJmY")[f])) > 1e-9 * math.fsum(np.abs(case.species_field(0, "phiJmY")[f]))
    case.close(); dev.close()


# ---- 4. the species balance closes ------------------------------------------------------------------------------------------------------------
def inlet_species_bcs(nS, inert):
    """every species fixedValue at the inlet (patch 0), within [0.05, 0.9], adding up to 1"""
    v = [0.06 + 0.01 * i for i in range(nS)]
    v[inert] = 1.0 - (sum(v) - v[inert])
    return [(i, 0, ("fixedValue", v[i])) for i in range(nS)]


@pytest.mark.parametrize("branch,stencil,adjust", [("explicit", "GaussVolPoint", 0), ("explicit", "GaussVolPoint", 1), ("explicit", "reduced", 0),
                                                   ("explicit", "reduced", 1), ("implicit", "GaussVolPoint", 0)])
def test_patch_fluxes_close_the_balance_of_every_species(branch, stencil, adjust):
    """after each of 5 steps on an open 10 x 9 x 8 box, for every species (the inert one included)
        |M_i^n - M_i^(n-1) + deltaT_n sum_patches Phi_i| <= (nCells + nFaces) 2^-52 (sum |rho Y_i V| + deltaT_n sum_faces |F_i|)
    F_i the per-face flux of consumed_terms over all patch faces; on the implicit branch (implicitTol 1e-14) plus the final residuals
    species_implicit_info reports times sum V / deltaT_n (the inert species: those of all transported ones).  No clip is active: every Y_i
    starts within [0.05, 0.9], and the sampled minima and the sum defect say so after every step."""
    mesh = q.PolyMesh.box(10, 9, 8)
    nS, inert = 6, 2
    implicit = branch == "implicit"
    C = mesh.array("C").reshape(-1, 3)
    Y0 = composition(C, nS, inert)
    assert all(y.min() >= 0.05 and y.max() <= 0.9 for y in Y0)
    dev, case = species_case(mesh, nS, inert, bc_fn=io_bcs, species_bcs=inlet_species_bcs(nS, inert), Y0=Y0, implicit=implicit, keep=True,
                             stencil=stencil, adjustTimeStep=adjust, maxCo=0.3)
    names = [f"S{i}" for i in range(nS)]
    m = case.monitor(patches=range(6), species=True)
    V = mesh.array("V")
    nif = mesh.nInternalFaces
    bfaces = np.arange(nif, mesh.nFaces)
    m.sample()
    prev = m.read()["speciesMass"]
    some_flux = 0.0
    for step in range(1, 6):
        case.updateFluxes()
        phiJm = case.field("phiJm")
        Yb_old = [case.species_field(i, "Y.boundary") for i in range(nS)]
        case.step(1)
        m.sample()
        s = m.read()
        dt = case.info()["deltaT"]
        assert s["speciesFluxState"] == (2 if implicit else 1) and s["step"] == step and s["deltaT"] == dt
        assert s["speciesMin"].min() > 0.0 and s["speciesSumDefect"] <= 1e-13, (s["speciesMin"], s["speciesSumDefect"])     # no clip was active
        rho = case.field("rho")
        resid = {}
        if implicit:
            info = case.species_implicit_info()
            assert info["unconvergedSteps"] == 0
            resid = {names.index(k): v["final"] for k, v in info["species"].items()}
            resid[inert] = sum(resid.values())
        now = s["speciesMass"]
        Phi = s["speciesPatchFlux"].sum(axis=0)
        for i in range(nS):
            absQ = math.fsum(np.abs(rho * case.species_field(i) * V))
            absF = math.fsum(np.abs(consumed_terms(case, mesh, i, inert, nS, phiJm, Yb_old, implicit, bfaces).sum(axis=0)))
            defect = abs(now[i] - prev[i] + dt * Phi[i])
            bound = (mesh.nCells + mesh.nFaces) * EPS * (absQ + dt * absF)
            if implicit:
                bound += resid[i] * math.fsum(V) / dt
            print(f"{branch} {stencil} adjust {adjust} step {step} species {i}: M {now[i]!r} dM {now[i] - prev[i]:.6e} dt*Phi {dt * Phi[i]:.6e} "
                  f"defect {defect:.3e} bound {bound:.3e}" + (f" (residual {resid[i]:.3e})" if implicit else ""))
            assert defect <= bound, (branch, stencil, adjust, step, i, defect, bound)
            some_flux = max(some_flux, abs(Phi[i]))
        prev = now
    assert some_flux > 0.0                                   # an open box
    if adjust:
        assert case.info()["deltaT"] != 1e-3
    case.close(); dev.close()


# ---- 5. flux state -----------------------------------------------------------------------------------------------------------------------------
def test_species_flux_state_follows_the_species_assembly():
    """qgd_capi.cpp: qgd_case_set_fields and qgd_case_set_species_fields clear spFluxesValid, the species advance of a step sets it,
    qgd_case_update_fluxes assembles the flow's fluxes only and leaves it as it is"""
    mesh = q.PolyMesh.box(6, 5, 4)
    dev, case = species_case(mesh, 4, 1, bc_fn=io_bcs)
    m = case.monitor(patches=[0, 1], species=True)
    s = m.read(m.sample())
    assert s["speciesFluxState"] == 0 and s["fluxState"] == 0 and np.isnan(s["speciesPatchFlux"]).all() and s["speciesPatchFlux"].shape == (2, 4)
    assert np.isfinite(s["speciesMass"]).all()
    case.updateFluxes()
    s = m.read(m.sample())
    assert s["fluxState"] == 1 and s["speciesFluxState"] == 0 and np.isnan(s["speciesPatchFlux"]).all()
    case.step(1)
    s = m.read(m.sample())
    assert s["speciesFluxState"] == 1 and np.isfinite(s["speciesPatchFlux"]).all()
    case.updateFluxes()
    s2 = m.read(m.sample())
    assert s2["speciesFluxState"] == 1 and np.isfinite(s2["speciesPatchFlux"]).all()
    case.set_species_field(0, case.species_field(0))
    s = m.read(m.sample())
    assert s["speciesFluxState"] == 0 and np.isnan(s["speciesPatchFlux"]).all()
    case.close(); dev.close()


# ---- 6. shards and cyclic copies -----------------------------------------------------------------------------------------------------------------
def test_three_shards_on_one_device_add_up_to_the_unsharded_species_block():
    g = make_mesh("box654_poly")
    n, nS, inert = g.nCells, 6, 2
    C = g.array("C").reshape(-1, 3)
    fields = cases.box_initial_fields(C)
    Y0 = composition(C, nS, inert)
    probes = [5, 60, 110]
    dev, case = species_case(g, nS, inert, bc_fn=io_bcs, Y0=Y0, fields=fields)
    mon = case.monitor(patches=range(6), probes=probes, species=True)
    mon.sample()
    whole = mon.read()
    rho, V = case.field("rho"), g.array("V")
    parts, keep = [], []
    for r in range(3):
        sh = g.shard(3, r)
        cg = sh.array("cellGlobal")
        own = np.nonzero((cg >= (n * r) // 3) & (cg < (n * (r + 1)) // 3))[0]
        d, c = species_case(sh, nS, inert, bc_fn=io_bcs, Y0=Y0, fields=fields, cells=cg, halo=True)    # explicit branch, QGD_SPECIES_HALO
        where = {int(cg[i]): int(i) for i in own}
        mo = c.monitor(patches=range(6), probes=[where.get(x, -1) for x in probes], species=True)
        mo.sample()
        s = mo.read()
        assert s["ownedCells"] == own.size and s["ownedCells"] < sh.nCells
        check_species_cells(s, c, sh.array("V"), nS, owned=own, labels=cg[own], what=f"shard {r}")
        s.pop("raw"); s.pop("speciesRaw")
        parts.append(s)
        keep.append((d, c))
    tot = combine(parts)
    for key in ("speciesMin", "speciesMinCell", "speciesMax", "speciesMaxCell", "speciesProbes", "min", "minCell", "probes"):
        assert np.array_equal(tot[key], whole[key]), (key, tot[key], whole[key])
    assert tot["speciesSumDefect"] == whole["speciesSumDefect"] and tot["speciesNonFinite"] == 0 and tot["speciesFluxState"] == 0
    for i in range(nS):
        terms = rho * Y0[i] * V
        sum_ok(tot["speciesMass"][i], terms, f"shards: mass of species {i}", n=terms.size + 3)
        sum_ok(whole["speciesMass"][i], terms, f"unsharded: mass of species {i}")
    for d, c in keep:
        c.close(); d.close()
    case.close(); dev.close()


def test_stepped_shards_report_the_patch_fluxes_of_the_unsharded_case():
    """three shards stepped with their state messages (tests/test_species_halo_gpu.py drives them) against the unsharded case after the
    same two steps.  The shards' fields agree with the unsharded ones to that file's bar, 1e-12 of the field's scale, not bit for bit, and
    a face flux is a difference of neighbouring values over a cell width (about 1/6 here): the totals are compared within 1e-10 of
    sum |face flux| (1e-12, times 6 for the gradient, with a margin of 16 for the terms of a flux)"""
    from test_species_halo_gpu import COMPOSITIONS, SETUPS, Shards, inlet_bcs, mesh_of as halo_mesh_of, put_species
    kind, stencil, nS = "box654_poly", "GaussVolPoint", 6
    g = halo_mesh_of(kind)
    _, init_fn, opt = SETUPS[kind]
    bc_fn = inlet_bcs(g)
    Y_fn, Sc, inlet = COMPOSITIONS[nS]
    C = g.array("C").reshape(-1, 3)
    dev = q.Device(g, fused_tables=False)
    case = q.QGDFoamCase(dev, q.default_options(stencil=stencil, **opt))
    bc_fn(case)
    put_species(case, Y_fn(C), Sc, inlet, keep_fluxes=True)
    case.set_fields(*init_fn(C))
    mon = case.monitor(patches=range(6), species=True)
    case.step(2)
    whole = mon.read(mon.sample())
    nif = g.nInternalFaces
    absF = [math.fsum(np.abs(case.species_field(i, "phiJmY")[nif:]) + np.abs(case.species_field(i, "diffusiveFlux")[nif:])) for i in range(nS)]
    case.updateFluxes()              # (after the sample; the mass flux of the state reached: its magnitude enters the inert species' bound)
    absF[2] = sum(absF) + math.fsum(np.abs(case.field("phiJm")[nif:]))
    sh = Shards(g, 3, stencil, bc_fn, init_fn, opt, nS)
    mons = [c.monitor(patches=range(6), species=True) for c in sh.cs]
    sh.run(2, False)
    parts = []
    for mo in mons:
        s = mo.read(mo.sample())
        s.pop("raw"); s.pop("speciesRaw")
        parts.append(s)
    tot = combine(parts)
    assert tot["ownedCells"] == g.nCells and tot["speciesFluxState"] == 1 and whole["speciesFluxState"] == 1
    for i in range(nS):
        d = np.abs(tot["speciesPatchFlux"][:, i] - whole["speciesPatchFlux"][:, i]).max()
        print(f"species {i}: patch totals of the shards differ from the unsharded ones by {d:.3e}, bound {1e-10 * absF[i]:.3e}")
        assert d <= 1e-10 * absF[i] and np.abs(whole["speciesPatchFlux"][:, i]).max() > 0
        assert abs(tot["speciesMass"][i] - whole["speciesMass"][i]) <= 1e-11 * abs(whole["speciesMass"][i])
    sh.close()
    case.close(); dev.close()


def test_copies_behind_cyclic_halves_are_not_counted():
    g = q.PolyMesh.box(10, 8, 6, patch_types=[L.PATCH_CYCLIC, L.PATCH_CYCLIC, G, G, G, G])
    ext = g.unroll_cyclic()
    n, nS, inert = g.nCells, 5, 0
    cg = ext.array("cellGlobal")
    C = g.array("C").reshape(-1, 3)
    sbcs = [(1, 2, ("fixedValue", 0.2)), (3, 3, ("fixedValue", 0.1))]
    dev, case = species_case(ext, nS, inert, species_bcs=sbcs, Y0=composition(C, nS, inert), fields=cases.box_initial_fields(C), cells=cg, halo=True, keep=True)
    with pytest.raises(q.QgdError, match="cyclic patch"):
        case.monitor(patches=[0], species=True)
    m = case.monitor(patches=[2, 3, 4, 5], probes=[n - 1], species=True)
    case.updateFluxes()
    phiJm = case.field("phiJm")
    Yb_old = [case.species_field(i, "Y.boundary") for i in range(nS)]
    case.step(1)
    m.sample()
    s = m.read()
    assert ext.nCells > n and s["ownedCells"] == n
    check_species_cells(s, case, ext.array("V"), nS, owned=np.arange(n), what="cyclic")
    check_species_probes(s, case, [n - 1], nS)
    ps, pz, own = ext.array("patchStart"), ext.array("patchSize"), ext.array("owner")

    def real_faces(pa):
        f = np.arange(ps[pa], ps[pa] + pz[pa])
        return f[own[f] < n]
    assert real_faces(2).size == 60 and pz[2] > 60          # the copies own faces of the patch too
    check_species_patches(s, case, ext, [2, 3, 4, 5], nS, inert, phiJm, Yb_old, False, faces_of=real_faces, what="cyclic")
    case.close(); dev.close()


# ---- 7. repeatability and non-interference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("implicit", [False, True])
def test_sampling_is_repeatable_and_leaves_the_run_as_it_was(implicit):
    mesh = q.PolyMesh.box(12, 10, 8)
    nS, inert = 6, 3
    kw = dict(bc_fn=io_bcs, species_bcs=inlet_species_bcs(nS, inert), implicit=implicit)
    dev, case = species_case(mesh, nS, inert, **kw)
    case.step(5)
    plain = {f: case.field(f) for f in ("rho", "U", "p", "e", "rhoE")}
    plainY = [case.species_field(i) for i in range(nS)]
    case.close(); dev.close()

    dev, case = species_case(mesh, nS, inert, **kw)
    m = case.monitor(probes=[0, 500], patches=range(6), species=True)
    rows = []
    for _ in range(5):
        case.step(1)
        slot = m.sample()
        rows.append((m.read_species_raw(slot), m.read_raw(slot)[0]))
    for f, want in plain.items():
        assert np.array_equal(case.field(f), want), (implicit, f)
    for i in range(nS):
        assert np.array_equal(case.species_field(i), plainY[i]), (implicit, i)
    slot_a, slot_b = m.sample(), m.sample()
    a, b = m.read_species_raw(slot_a), m.read_species_raw(slot_b)
    assert a.tobytes() == b.tobytes() == rows[-1][0].tobytes()
    assert m.read_raw(slot_a)[0].tobytes() == m.read_raw(slot_b)[0].tobytes() == rows[-1][1].tobytes()
    case.close(); dev.close()


def test_a_monitor_without_the_species_block_is_the_flow_monitor_it_was():
    mesh = q.PolyMesh.box(8, 7, 6)
    dev, case = species_case(mesh, 4, 1, bc_fn=io_bcs)
    flow = case.monitor(probes=[0, 7, -1], patches=[0, 5])
    both = case.monitor(probes=[0, 7, -1], patches=[0, 5], species=True)
    assert flow.offsets == both.offsets == [0, 8, 16, 36, 57] and flow.n_doubles == both.n_doubles == 57 + 18 and L.ABI_VERSION == 9
    assert not flow.species and flow.species_offsets is None and flow.species_doubles == 0
    case.step(2)
    sf, sb = flow.sample(), both.sample()
    raw_f, raw_b = flow.read_raw(sf)[0], both.read_raw(sb)[0]
    assert raw_f.tobytes() == raw_b.tobytes()               # the flow block is the same with the species block behind it
    s = flow.read(flow.sample())
    assert not any(k.startswith("species") or k == "nSpecies" for k in s)
    with pytest.raises(q.QgdError, match="not enabled") as ei:
        flow.read_species_raw(sf)
    assert ei.value.code == L.ERR_INVALID
    case.close(); dev.close()


def test_slots_are_read_two_samples_late():
    mesh = q.PolyMesh.box(8, 7, 6)
    dev, case = species_case(mesh, 5, 2, bc_fn=io_bcs, species_bcs=inlet_species_bcs(5, 2))
    m = case.monitor(probes=[10], species=True)
    with pytest.raises(q.QgdError, match="never sampled"):
        m.read_species_raw(2)
    y10, got = [], []
    for step in range(1, 9):
        case.step(1)
        y10.append([case.species_field(i)[10] for i in range(5)])
        assert m.sample() == (step - 1) % 4
        if step >= 3:
            got.append(m.read())                  # the oldest unread sample: two behind
            assert got[-1]["step"] == step - 2
    got += [m.read(), m.read()]
    assert [s["step"] for s in got] == list(range(1, 9))
    assert [list(s["speciesProbes"][0]) for s in got] == y10
    case.close(); dev.close()


# ---- 8. refusals by name ---------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_their_reason():
    mesh = q.PolyMesh.box(4, 3, 2)
    dev = q.Device(mesh, fused_tables=False)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3))
    case.set_fields(*cases.box_initial_fields(mesh.array("C").reshape(-1, 3)))
    with pytest.raises(q.QgdError, match="carries no species") as ei:
        case.monitor(species=True)
    assert ei.value.code == L.ERR_INVALID and "qgd_monitor_enable_species" in str(ei.value)
    plain = case.monitor(probes=[0])
    off, n = (L.C.c_int64 * 5)(), L.C.c_int64()
    assert L.lib.qgd_monitor_species_layout(plain._h, off, L.C.byref(n)) == L.ERR_INVALID and b"not enabled" in L.lib.qgd_last_error()
    plain.sample()
    assert L.lib.qgd_monitor_species_read(plain._h, 0, np.zeros(64).ctypes.data_as(L.c_double_p), 64) == L.ERR_INVALID
    assert b"not enabled" in L.lib.qgd_last_error() and b"qgd_monitor_species_read" in L.lib.qgd_last_error()
    case.close(); dev.close()

    dev, case = species_case(mesh, 3, 0)
    m = case.monitor(probes=[0], species=True)
    assert L.lib.qgd_monitor_enable_species(m._h) == 0       # once more: nothing happens
    slot = m.sample()
    small = np.zeros(m.species_doubles - 1)
    with pytest.raises(q.QgdError, match="output too small") as ei:
        L.check(L.lib.qgd_monitor_species_read(m._h, slot, small.ctypes.data_as(L.c_double_p), small.size), "qgd_monitor_species_read")
    assert ei.value.code == L.ERR_INVALID and str(m.species_doubles) in str(ei.value)
    with pytest.raises(q.QgdError, match="slot must be"):
        m.read_species_raw(4)
    late = case.monitor(probes=[0])
    late.sample()
    with pytest.raises(q.QgdError, match="before the monitor's first") as ei:
        L.check(L.lib.qgd_monitor_enable_species(late._h), "qgd_monitor_enable_species")
    assert ei.value.code == L.ERR_INVALID
    raw = m._handle.value
    case.close()
    assert L.lib.qgd_monitor_enable_species(raw) == L.ERR_INVALID and b"freed with its case" in L.lib.qgd_last_error()
    dev.close()


# ---- 9. the application -----------------------------------------------------------------------------------------------------------------------
def test_application_writes_what_the_monitor_reads(tmp_path):
    from qgdsolver_amd import QGDFoam
    case_dir = str(tmp_path)
    write_species_case(case_dir)
    names = SPECIES["names"]
    locs = [(0.25, 0.5, 0.3), (0.8, 0.7, 0.6), (9.0, 9.0, 9.0)]
    with open(os.path.join(case_dir, "system", "controlDict"), "a") as f:
        f.write("functions\n{\n"
                "    wake { type probes; fields (O2 p H2O); probeLocations (" + " ".join("(%r %r %r)" % x for x in locs) + "); writeInterval 2; }\n"
                "    extremes { type fieldMinMax; fields (p O2 N2); writeInterval 2; }\n"
                "    budget { type qgdSpeciesIntegrals; writeInterval 2; }\n"
                "    ends { type qgdSpeciesPatchFluxes; patches (xMax xMin); writeInterval 2; }\n"
                "    flow { type qgdIntegrals; writeInterval 2; }\n"
                "    odd { type probes; fields (CO2); probeLocations ((0.5 0.5 0.5)); }\n"
                "}\n")
    lines = []
    dev, case, _ = QGDFoam.run(case_dir, n_steps=6, write=False, log=lines.append)
    case.close(); dev.close()
    assert sum("'odd'" in x and "field 'CO2' is not served" in x for x in lines) == 1
    assert sum("probe 2 is outside the mesh" in x for x in lines) == 1

    dev, case = ff.load_case(case_dir)
    cells = case.mesh.find_cells(locs)
    assert cells[0] >= 0 and cells[1] >= 0 and cells[2] == -1
    pn = case.mesh.patch_names
    m = case.monitor(probes=cells, patches=[pn.index("xMax"), pn.index("xMin")], species=True)
    want = []
    for _ in range(3):
        case.step(2)
        m.sample()
        want.append(m.read())
    C = case.mesh.array("C").reshape(-1, 3)
    case.close(); dev.close()
    post = os.path.join(case_dir, "postProcessing")

    def table(*path):
        return np.atleast_2d(np.loadtxt(os.path.join(post, *path), comments="#"))

    for name in ("O2", "H2O"):
        text = open(os.path.join(post, "wake", "0", name)).read().splitlines()
        assert text[2].endswith("# Not Found") and text[4] == "# Time"
        rows = np.array([[float(x) for x in ln.split()] for ln in text if not ln.startswith("#")])
        assert rows.shape == (3, 4)
        for r, s in zip(rows, want):
            assert r[0] == s["time"] and np.array_equal(r[1:], s["speciesProbes"][:, names.index(name)], equal_nan=True)
    rows = table("wake", "0", "p")
    for r, s in zip(rows, want):
        assert np.array_equal(r[1:], s["probes"][:, 4], equal_nan=True)
    rows = table("extremes", "0", "fieldMinMax.dat")
    assert rows.shape == (3, 31)
    for r, s in zip(rows, want):
        blocks = [(s["min"][1], s["minCell"][1], s["max"][1], s["maxCell"][1])]
        blocks += [(s["speciesMin"][k], s["speciesMinCell"][k], s["speciesMax"][k], s["speciesMaxCell"][k]) for k in (names.index("O2"), names.index("N2"))]
        for j, (lo, lo_c, hi, hi_c) in enumerate(blocks):
            blk = r[1 + 10 * j:11 + 10 * j]
            assert blk[0] == lo and blk[1] == lo_c and np.array_equal(blk[2:5], C[lo_c])
            assert blk[5] == hi and blk[6] == hi_c and np.array_equal(blk[7:10], C[hi_c])
    head = open(os.path.join(post, "budget", "0", "speciesIntegrals.dat")).read().splitlines()[1]
    assert head.split("\t") == ["# Time"] + [f"mass({n})" for n in names] + ["sumDefect", "nonFiniteCells", "firstNonFiniteCell"]
    rows = table("budget", "0", "speciesIntegrals.dat")
    assert rows.shape == (3, 7)
    for r, s in zip(rows, want):
        assert r[0] == s["time"] and np.array_equal(r[1:4], s["speciesMass"]) and r[4] == s["speciesSumDefect"] and r[5] == 0 and r[6] == -1
    rows = table("ends", "0", "speciesPatchFluxes.dat")
    assert rows.shape == (3, 7)
    for r, s in zip(rows, want):
        assert r[0] == s["time"] and np.array_equal(r[1:4], s["speciesPatchFlux"][0]) and np.array_equal(r[4:7], s["speciesPatchFlux"][1])
    assert np.abs(rows[:, 4:7]).min() > 0            # every species enters through the inlet
    rows = table("flow", "0", "volIntegrals.dat")
    for r, s in zip(rows, want):
        assert np.array_equal(r[1:9], s["integrals"])
