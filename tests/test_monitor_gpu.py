"""Run monitors on the device (qgd_monitor_*, qgdsolver_amd/csrc/qgd_monitor.hip): integrals, extrema, probes and patch flux totals
against numpy on the case's own fields, the discrete balance they close, ghosts, non-interference, refusals and the application.

Sums are compared with math.fsum of their terms under the bound n * 2^-52 * sum |term| (n terms), which holds for every order
of summation; extrema, labels and probe values of stored fields exactly; T, |U|, Mach to 1e-14 relative (at most four rounded
operations each)."""
import math
import os

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd import foamfile as ff
import cases
from test_foamfile import write_step_case
from util import assert_path, make_mesh

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
G, E = L.PATCH_GENERIC, L.PATCH_EMPTY


def sum_ok(got, terms, what, n=None):
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    n = terms.size if n is None else n
    exact = math.fsum(terms)
    bound = n * EPS * math.fsum(np.abs(terms))
    print(f"{what}: got {got!r} exact {exact!r} |diff| {abs(got - exact):.3e} bound {bound:.3e}")
    assert abs(got - exact) <= bound, (what, got, exact, abs(got - exact), bound)


def io_bcs(case):
    """inflow through patch 0, outflow through patch 1, the rest zeroGradient: open, and no mid-step exchange on shards"""
    case.set_bc(0, U=("fixedValue", (0.1, 0.0, 0.0)), T=("fixedValue", 1.05), p=("zeroGradient", None))
    case.set_bc(1, U=("zeroGradient", None), T=("zeroGradient", None), p=("fixedValue", 1.0))


def open_case(mesh, fused_tables=False, bc_fn=None, fields=None, **opt):
    opt = dict(dict(stencil="GaussVolPoint" if mesh.nGeometricD == 3 else "leastSquares", deltaT=1e-3, mu=1e-3), **opt)
    dev = q.Device(mesh, fused_tables=fused_tables)
    case = q.QGDFoamCase(dev, q.default_options(**opt))
    if bc_fn:
        bc_fn(case)
    U, T, p = fields if fields is not None else cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    return dev, case


def check_cells(s, case, V, owned=None, labels=None, what=""):
    """integrals and extrema of a sample against numpy over the owned cells of the case's fields"""
    owned = np.arange(V.size) if owned is None else owned
    labels = owned if labels is None else labels
    rho, U, p, e, rE, c = (case.field(f)[owned] for f in ("rho", "U", "p", "e", "rhoE", "c"))
    V = V[owned]
    ke = 0.5 * (U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1] + U[:, 2] * U[:, 2])
    assert s["ownedCells"] == owned.size and s["nonFinite"] == 0 and s["firstNonFinite"] == -1
    sum_ok(s["volume"], V, what + " volume")
    sum_ok(s["mass"], rho * V, what + " mass")
    for k in range(3):
        sum_ok(s["momentum"][k], rho * U[:, k] * V, what + f" momentum {k}")
    sum_ok(s["totalEnergy"], rE * V, what + " rhoE")
    sum_ok(s["internalEnergy"], rho * e * V, what + " rho e")
    sum_ok(s["kineticEnergy"], rho * ke * V, what + " kinetic")
    magU = np.sqrt(2.0 * ke)
    Cv = case.options.Cv
    for k, (name, a, exact) in enumerate((("rho", rho, True), ("p", p, True), ("T", e / Cv, False), ("magU", magU, False), ("Mach", magU / c, False))):
        for val, cell, arg in (("min", "minCell", np.argmin), ("max", "maxCell", np.argmax)):
            i = int(arg(a))                       # numpy's first occurrence: the lowest label of a tie (labels ascend with position)
            got, at = s[val][k], int(s[cell][k])
            print(f"{what} {val} {name}: got {got!r} at {at}, numpy {a[i]!r} at {labels[i]}")
            if exact:
                assert got == a[i] and at == labels[i], (what, val, name, got, a[i], at, labels[i])
            else:
                assert abs(got - a[i]) <= 1e-14 * abs(a[i]), (what, val, name, got, a[i])
                j = int(np.nonzero(labels == at)[0][0])      # the cell named holds that value (a rounding may move a near-tie)
                assert abs(a[j] - a[i]) <= 1e-14 * abs(a[i]), (what, val, name, at, labels[i])


def check_probes(s, case, cells):
    rho, U, p, e = (case.field(f) for f in ("rho", "U", "p", "e"))
    for row, c in zip(s["probes"], cells):
        if c < 0:
            assert np.isnan(row).all()
            continue
        assert row[0] == rho[c] and np.array_equal(row[1:4], U[c]) and row[4] == p[c] and row[6] == e[c]
        assert abs(row[5] - e[c] / case.options.Cv) <= 1e-14 * abs(e[c] / case.options.Cv)


# ---- 1. against numpy on case.field() ------------------------------------------------------------------------------------------------
def test_layout_and_grid_cap():
    dev, case = open_case(q.PolyMesh.box(2, 2, 2))
    m = case.monitor(probes=[0, 7, -1], patches=[0, 5])
    assert m.offsets == [0, 8, 16, 36, 57] and m.n_doubles == 57 + 18 and m.grid_cap == 1024 and L.ABI_VERSION == 9
    case.close(); dev.close()


@pytest.mark.parametrize("kind", ["box111", "box5_3_17", "box488", "box257_1_1", "box654_poly", "box64_64_65", "tet433", "prism543", "mix643"])
def test_integrals_extrema_and_probes_against_numpy(kind):
    dims = {"box111": (1, 1, 1), "box5_3_17": (5, 3, 17), "box488": (4, 8, 8), "box257_1_1": (257, 1, 1), "box64_64_65": (64, 64, 65)}
    mesh = make_mesh(kind) if kind not in dims else q.PolyMesh.box(*dims[kind])
    assert {"box5_3_17": 255, "box488": 256, "box257_1_1": 257}.get(kind, mesh.nCells) == mesh.nCells
    dev, case = open_case(mesh)
    probes = sorted({0, mesh.nCells // 2, mesh.nCells - 1}) + [-1]
    m = case.monitor(probes=probes)
    if kind == "box64_64_65":
        assert mesh.nCells > m.grid_cap * 256       # lanes take a second trip
    case.step(3)
    m.sample()
    s = m.read()
    assert s["step"] == 3 and s["time"] == case.info()["time"] and s["deltaT"] == 1e-3
    check_cells(s, case, mesh.array("V"), what=kind)
    check_probes(s, case, probes)
    case.close(); dev.close()


# ---- 2. special values ---------------------------------------------------------------------------------------------------------------
def test_uniform_field_puts_every_extremum_at_the_first_owned_cell():
    mesh = q.PolyMesh.box(9, 8, 7)
    n = mesh.nCells
    dev, case = open_case(mesh, fields=(np.tile([0.1, 0.2, 0.3], (n, 1)), np.full(n, 1.1), np.full(n, 0.9)))
    m = case.monitor()
    m.sample()
    s = m.read()
    assert np.array_equal(s["minCell"], np.zeros(5)) and np.array_equal(s["maxCell"], np.zeros(5)), (s["minCell"], s["maxCell"])
    assert np.array_equal(s["min"], s["max"]) and s["min"][1] == 0.9
    case.close(); dev.close()
    # a shard: the first owned cell is not local cell 0, and its label is that of the unsharded mesh
    sh = mesh.shard(3, 1)
    cg = sh.array("cellGlobal")
    dev, case = open_case(sh, fields=(np.tile([0.1, 0.2, 0.3], (cg.size, 1)), np.full(cg.size, 1.1), np.full(cg.size, 0.9)))
    m = case.monitor()
    m.sample()
    s = m.read()
    first = n // 3
    assert first in cg and cg[0] < first
    assert np.array_equal(s["minCell"], np.full(5, first)) and np.array_equal(s["maxCell"], np.full(5, first)), (s["minCell"], first)
    assert s["ownedCells"] == (2 * n) // 3 - n // 3
    case.close(); dev.close()


def test_one_nan_cell_is_counted_named_and_kept_out_of_the_extrema():
    mesh = q.PolyMesh.box(7, 6, 5)
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    bad = 137
    T = T.copy()
    T[bad] = np.nan
    dev, case = open_case(mesh, fields=(U, T, p))
    m = case.monitor()
    m.sample()                                   # no step taken
    s = m.read()
    assert s["nonFinite"] == 1 and s["firstNonFinite"] == bad
    assert s["fluxState"] == 0
    others = np.delete(np.arange(mesh.nCells), bad)
    rho, pp = case.field("rho")[others], case.field("p")[others]
    assert s["min"][0] == rho.min() and s["minCell"][0] == others[np.argmin(rho)]
    assert s["max"][0] == rho.max() and s["maxCell"][0] == others[np.argmax(rho)]
    assert s["min"][1] == pp.min() and s["max"][1] == pp.max() and s["maxCell"][1] == others[np.argmax(pp)]
    assert bad not in s["minCell"] and bad not in s["maxCell"] and np.isfinite(s["min"]).all() and np.isfinite(s["max"]).all()
    # the sums that meet the cell are NaN; the volume is not
    assert np.isnan(s["mass"]) and np.isnan(s["momentum"]).all() and np.isnan(s["totalEnergy"]) and np.isnan(s["internalEnergy"])
    sum_ok(s["volume"], mesh.array("V"), "volume next to a NaN cell")
    case.close(); dev.close()


# ---- 3. balance ------------------------------------------------------------------------------------------------------------------------
BALANCE = [pytest.param(arm, adjust, None, id=f"{arm}-{adjust}") for arm, adjust in (("fused", 0), ("kernels", 0), ("kernels", 1), ("fusedAdjust", 1))]
BALANCE += [pytest.param(arm, 0, kind, id=f"{arm}-0-{kind}") for kind in ("tet433", "prism543", "mix643") for arm in ("fused", "kernels")]
BALANCE += [pytest.param(arm, 0, "ref533", id=f"{arm}-0-ref533") for arm in ("fused", "kernels")]      # 2:1 refined: cells of 6 to 24 faces


@pytest.mark.parametrize("arm,adjust,kind", BALANCE)
def test_patch_fluxes_close_the_balance_of_mass_momentum_and_energy(arm, adjust, kind):
    """|Q_n - Q_(n-1) + deltaT_n sum F| <= (nCells + nFaces) 2^-52 (sum |q V| + deltaT_n sum |F|) after each of 5 steps, for mass, the three
    momentum components and rho E; F over all patches, deltaT_n from info()"""
    mesh = make_mesh(kind) if kind else q.PolyMesh.box(10, 9, 8)
    dev, case = open_case(mesh, fused_tables=False if arm == "kernels" else "any", bc_fn=io_bcs, adjustTimeStep=adjust, maxCo=0.3)
    assert_path(case, arm, arm)
    m = case.monitor(patches=range(6))
    V = mesh.array("V")
    nif = mesh.nInternalFaces
    m.sample()
    prev = m.read()["integrals"][1:6]
    for step in range(1, 6):
        # the face fields of the assembly the step is about to repeat: their magnitudes enter the bound
        case.updateFluxes()
        absF = [np.abs(case.field("phiJm")[nif:])]
        absF += [np.abs(case.field("phiJmU")[nif:, k]) + np.abs(case.field("phiP")[nif:, k]) + np.abs(case.field("phiPi")[nif:, k]) for k in range(3)]
        absF += [np.abs(case.field("phiJmH")[nif:]) + np.abs(case.field("phiQ")[nif:]) + np.abs(case.field("phiPiU")[nif:])]
        case.step(1)
        m.sample()
        s = m.read()
        dt = case.info()["deltaT"]
        assert s["fluxState"] == 1 and s["step"] == step and s["deltaT"] == dt and s["time"] == case.info()["time"]
        rho, U, rE = case.field("rho"), case.field("U"), case.field("rhoE")
        absQ = [math.fsum(np.abs(rho * V))] + [math.fsum(np.abs(rho * U[:, k] * V)) for k in range(3)] + [math.fsum(np.abs(rE * V))]
        now = s["integrals"][1:6]
        F = s["patchFlux"].sum(axis=0)
        assert math.fsum(absF[0]) > 0 and np.abs(s["patchFlux"][:, 0]).sum() > 0      # an open box
        for k, name in enumerate(("mass", "momentum x", "momentum y", "momentum z", "rho E")):
            defect = abs(now[k] - prev[k] + dt * F[k])
            bound = (mesh.nCells + mesh.nFaces) * EPS * (absQ[k] + dt * math.fsum(absF[k]))
            print(f"{arm} adjust {adjust} step {step} {name}: Q {now[k]!r} dQ {now[k] - prev[k]:.6e} dt*F {dt * F[k]:.6e} defect {defect:.3e} bound {bound:.3e}")
            assert defect <= bound, (arm, adjust, step, name, defect, bound)
        prev = now
    if adjust:
        assert case.info()["deltaT"] != 1e-3
    case.close(); dev.close()


# ---- 4. patch totals against the face fields ------------------------------------------------------------------------------------------
def check_patches(s, case, mesh, patches, faces_of=None, what=""):
    """after update_fluxes() then step(1): the monitor's totals against the face fields of that assembly"""
    ps, pz = mesh.array("patchStart"), mesh.array("patchSize")
    f1 = {n: case.field(n) for n in ("phiJm", "phiJmH", "phiQ", "phiPiU")}
    f3 = {n: case.field(n) for n in ("phiJmU", "phiP", "phiPi")}
    Sf, mag = mesh.array("Sf").reshape(-1, 3), mesh.array("magSf")
    pb = case.field("p.boundary")
    nif = mesh.nInternalFaces
    for row, pa in enumerate(patches):
        f = np.arange(ps[pa], ps[pa] + pz[pa]) if faces_of is None else faces_of(pa)
        tag = f"{what} patch {pa} ({f.size} faces)"
        sum_ok(s["patchArea"][row], mag[f], tag + " area")
        sum_ok(s["patchFlux"][row, 0], f1["phiJm"][f], tag + " mass")
        for k in range(3):
            sum_ok(s["patchFlux"][row, 1 + k], np.concatenate([f3["phiJmU"][f, k], f3["phiP"][f, k], -f3["phiPi"][f, k]]), tag + f" momentum {k}")
        sum_ok(s["patchFlux"][row, 4], np.concatenate([f1["phiJmH"][f], f1["phiQ"][f], -f1["phiPiU"][f]]), tag + " energy")
        for k in range(3):
            sum_ok(s["patchPressureForce"][row, k], pb[f - nif] * Sf[f, k], tag + f" p Sf {k}")


@pytest.mark.parametrize("kind", ["box111", "box20_17_3", "box654_poly", "box257_257_1", "tet433", "prism543", "mix643", "ref533"])
def test_patch_totals_against_the_face_fields(kind):
    dims = {"box111": (1, 1, 1), "box20_17_3": (20, 17, 3), "box257_257_1": (257, 257, 1)}
    mesh = q.PolyMesh.box(*dims[kind]) if kind in dims else make_mesh(kind)
    dev, case = open_case(mesh, bc_fn=io_bcs)
    patches = [5, 0, 1, 2, 3, 4, 0]                  # any order, one of them twice
    m = case.monitor(patches=patches)
    m.sample()
    s0 = m.read()
    assert s0["fluxState"] == 0 and np.isnan(s0["patchFlux"]).all() and not np.isnan(s0["patchArea"]).any() and not np.isnan(s0["patchPressureForce"]).any()
    case.updateFluxes()
    case.step(1)
    m.sample()
    s = m.read()
    assert s["fluxState"] == 1
    if kind == "box20_17_3":
        assert mesh.array("patchSize")[4] == 340     # more than one chunk of 256
    if kind == "box257_257_1":
        assert list(mesh.array("patchSize")[4:6]) == [66049] * 2     # 259 chunks: the fold's threads take a second trip over a patch's rows
    if kind == "box111":
        assert list(mesh.array("patchSize")) == [1] * 6
    check_patches(s, case, mesh, patches, what=kind)
    assert np.array_equal(s["patchFlux"][1], s["patchFlux"][6])
    case.close(); dev.close()


def test_two_dimensional_mesh_reports_its_real_patches_and_refuses_the_empty_ones_by_name():
    mesh = make_mesh("plane2d_jitter")
    dev, case = open_case(mesh, bc_fn=io_bcs)
    with pytest.raises(q.QgdError, match="empty patch") as ei:
        case.monitor(patches=[0, 4])
    assert ei.value.code == L.ERR_INVALID and "patch 4" in str(ei.value)
    m = case.monitor(patches=[0, 1, 2, 3])
    case.updateFluxes()
    case.step(1)
    m.sample()
    s = m.read()
    check_patches(s, case, mesh, [0, 1, 2, 3], what="plane2d_jitter")
    check_cells(s, case, mesh.array("V"), what="plane2d_jitter")
    case.close(); dev.close()


def test_implicit_diffusion_reports_the_mass_flux_only():
    mesh = q.PolyMesh.box(6, 5, 4)
    dev, case = open_case(mesh, bc_fn=io_bcs, implicitDiffusion=1)
    m = case.monitor(patches=[0, 1])
    case.step(1)
    m.sample()
    s = m.read()
    assert s["fluxState"] == 2 and np.isfinite(s["patchFlux"][:, 0]).all() and np.abs(s["patchFlux"][:, 0]).sum() > 0
    assert np.isnan(s["patchFlux"][:, 1:]).all() and np.isfinite(s["patchArea"]).all()
    case.close(); dev.close()


# ---- 5. ghosts --------------------------------------------------------------------------------------------------------------------------
def test_three_shards_on_one_device_add_up_to_the_unsharded_monitor():
    g = make_mesh("box654_poly")
    n = g.nCells
    U, T, p = cases.box_initial_fields(g.array("C").reshape(-1, 3))
    patches = list(range(6))
    dev, case = open_case(g, bc_fn=io_bcs, fields=(U, T, p))
    mon = case.monitor(patches=patches, probes=[5, 60, 110])
    case.updateFluxes()
    mon.sample()
    whole = mon.read()
    ps, pz = g.array("patchStart"), g.array("patchSize")
    face_terms = {nme: case.field(nme) for nme in ("phiJm", "phiJmU", "phiP", "phiPi", "phiJmH", "phiQ", "phiPiU")}
    V = g.array("V")
    fields = {f: case.field(f) for f in ("rho", "U", "rhoE", "e")}
    parts, keep = [], []
    for r in range(3):
        sh = g.shard(3, r)
        cg = sh.array("cellGlobal")
        own = np.nonzero((cg >= (n * r) // 3) & (cg < (n * (r + 1)) // 3))[0]
        d, c = open_case(sh, bc_fn=io_bcs, fields=(U[cg], T[cg], p[cg]))      # (set_fields gives the ghost cells their values too)
        with pytest.raises(q.QgdError, match="halo patch") as ei:
            c.monitor(patches=[sh.nPatches - 1])
        assert ei.value.code == L.ERR_INVALID
        where = {int(cg[i]): int(i) for i in own}
        mo = c.monitor(patches=patches, probes=[where.get(x, -1) for x in (5, 60, 110)])
        c.updateFluxes()
        mo.sample()
        s = mo.read()
        assert s["ownedCells"] == own.size and s["ownedCells"] < sh.nCells
        check_cells(s, c, sh.array("V"), owned=own, labels=cg[own], what=f"shard {r}")
        s.pop("raw")
        parts.append(s)
        keep.append((d, c))
    from qgdsolver_amd.monitor import combine
    tot = combine(parts)
    assert tot["ownedCells"] == n
    # extrema: the unsharded ones, with the same labels of the unsharded mesh; the probes from the shard that owns the cell
    for key in ("min", "minCell", "max", "maxCell", "probes"):
        assert np.array_equal(tot[key], whole[key]), (key, tot[key], whole[key])
    rho, Uf, rE, e = fields["rho"], fields["U"], fields["rhoE"], fields["e"]
    ke = 0.5 * (Uf * Uf).sum(axis=1)
    for k, terms in enumerate([V, rho * V, rho * Uf[:, 0] * V, rho * Uf[:, 1] * V, rho * Uf[:, 2] * V, rE * V, rho * e * V, rho * ke * V]):
        sum_ok(tot["integrals"][k], terms, f"shards: integral {k}", n=terms.size + 3)
        sum_ok(whole["integrals"][k], terms, f"unsharded: integral {k}")
    for row, pa in enumerate(patches):
        f = np.arange(ps[pa], ps[pa] + pz[pa])
        cols = [face_terms["phiJm"][f]] + [np.concatenate([face_terms["phiJmU"][f, k], face_terms["phiP"][f, k], -face_terms["phiPi"][f, k]]) for k in range(3)]
        cols += [np.concatenate([face_terms["phiJmH"][f], face_terms["phiQ"][f], -face_terms["phiPiU"][f]])]
        for k, terms in enumerate(cols):
            sum_ok(tot["patchFlux"][row, k], terms, f"shards: patch {pa} flux {k}", n=terms.size + 3)
            sum_ok(whole["patchFlux"][row, k], terms, f"unsharded: patch {pa} flux {k}")
        sum_ok(tot["patchArea"][row], g.array("magSf")[f], f"shards: patch {pa} area", n=f.size + 3)
    for d, c in keep:
        c.close(); d.close()
    case.close(); dev.close()


@pytest.mark.parametrize("arm", ["fused", "kernels"])
def test_copies_behind_cyclic_halves_are_not_counted(arm):
    g = q.PolyMesh.box(10, 8, 6, patch_types=[L.PATCH_CYCLIC, L.PATCH_CYCLIC, G, G, G, G])
    ext = g.unroll_cyclic()
    n = g.nCells
    cg = ext.array("cellGlobal")
    U, T, p = cases.box_initial_fields(g.array("C").reshape(-1, 3))
    dev, case = open_case(ext, fused_tables="any" if arm == "fused" else False, fields=(U[cg], T[cg], p[cg]))
    assert case.fused_info()["fused"] == (arm == "fused")     # (the blocks of an unrolled mesh leave the copies' own faces out)
    with pytest.raises(q.QgdError, match="cyclic patch"):
        case.monitor(patches=[0])
    m = case.monitor(patches=[2, 3, 4, 5], probes=[n - 1])
    case.updateFluxes()
    case.step(1)
    m.sample()
    s = m.read()
    assert ext.nCells > n and s["ownedCells"] == n
    check_cells(s, case, ext.array("V"), owned=np.arange(n), what="cyclic " + arm)
    check_probes(s, case, [n - 1])
    ps, pz, own = ext.array("patchStart"), ext.array("patchSize"), ext.array("owner")

    def real_faces(pa):
        f = np.arange(ps[pa], ps[pa] + pz[pa])
        return f[own[f] < n]
    assert real_faces(2).size == 60 and pz[2] > 60          # the copies own faces of the patch too
    check_patches(s, case, ext, [2, 3, 4, 5], faces_of=real_faces, what="cyclic " + arm)
    assert abs(s["patchArea"][0] - 1.0) <= 60 * EPS
    case.close(); dev.close()


# ---- 6. non-interference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["fused", "kernels"])
def test_sampling_is_repeatable_and_leaves_the_run_as_it_was(arm):
    mesh = q.PolyMesh.box(12, 10, 8)
    tables = "any" if arm == "fused" else False
    dev, case = open_case(mesh, fused_tables=tables, bc_fn=io_bcs)
    assert_path(case, arm, arm)
    case.step(5)
    plain = {f: case.field(f) for f in ("rho", "U", "p", "e", "rhoE")}
    case.close(); dev.close()

    dev, case = open_case(mesh, fused_tables=tables, bc_fn=io_bcs)
    m = case.monitor(probes=[0, 500], patches=range(6))
    rows = []
    for _ in range(5):
        case.step(1)
        m.sample()
        rows.append(m.read_raw()[0])
    for f, want in plain.items():
        assert np.array_equal(case.field(f), want), (arm, f)
    # two samples of one state are bitwise equal; an odd number of fused steps left the records in the second pair of buffers
    a = m.read_raw(m.sample())[0]
    b = m.read_raw(m.sample())[0]
    assert a.tobytes() == b.tobytes() == rows[-1].tobytes()
    case.close(); dev.close()


def test_state_reads_the_same_whichever_path_produced_it():
    """the monitor's sums depend on the mesh and the specification only: the same records give the same bits under either device"""
    mesh = q.PolyMesh.box(12, 10, 8)
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    raws = []
    for tables in ("any", False):
        dev, case = open_case(mesh, fused_tables=tables, fields=(U, T, p))
        m = case.monitor(probes=[3])
        m.sample()
        raws.append(m.read_raw()[0])
        case.close(); dev.close()
    assert raws[0].tobytes() == raws[1].tobytes()


def test_slots_are_read_two_samples_late():
    mesh = q.PolyMesh.box(8, 7, 6)
    dev, case = open_case(mesh, bc_fn=io_bcs)
    m = case.monitor(probes=[10])
    with pytest.raises(q.QgdError, match="never sampled"):
        m.read(2)
    with pytest.raises(q.QgdError, match="slot must be"):
        m.sample(4)
    rho10, got = [], []
    for step in range(1, 9):
        case.step(1)
        rho10.append(case.field("rho")[10])
        assert m.sample() == (step - 1) % 4
        if step >= 3:
            got.append(m.read())                  # the oldest unread sample: two behind
            assert got[-1]["step"] == step - 2
    got += [m.read(), m.read()]
    assert [s["step"] for s in got] == list(range(1, 9))
    assert [s["probes"][0, 0] for s in got] == rho10
    with pytest.raises(ValueError):
        m.read()
    case.close(); dev.close()


# ---- 7. refusals and lifetime --------------------------------------------------------------------------------------------------------
def test_refusals_carry_their_reason():
    mesh = q.PolyMesh.box(4, 3, 2)
    dev = q.Device(mesh, fused_tables=False)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3))
    with pytest.raises(q.QgdError, match="qgd_case_set_fields first") as ei:
        case.monitor()
    assert ei.value.code == L.ERR_INVALID
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    for bad in (24, -2):
        with pytest.raises(q.QgdError, match="out of range") as ei:
            case.monitor(probes=[0, bad])
        assert ei.value.code == L.ERR_INVALID and f"cell label {bad}" in str(ei.value)
    with pytest.raises(q.QgdError, match="patch index 6") as ei:
        case.monitor(patches=[6])
    assert ei.value.code == L.ERR_INVALID
    m = case.monitor(probes=[0])
    with pytest.raises(q.QgdError, match="output too small"):
        L.check(L.lib.qgd_monitor_read(m._h, 0, np.zeros(4).ctypes.data_as(L.c_double_p), 4, None, None), "qgd_monitor_read")
    case.close(); dev.close()


def test_closing_the_case_first_frees_its_monitors_once():
    mesh = q.PolyMesh.box(4, 3, 2)
    dev, case = open_case(mesh)
    m1, m2 = case.monitor(probes=[1]), case.monitor(patches=[0])
    m1.sample()
    raw = m1._handle.value
    m2.close()                                   # one closed before its case, one after
    case.close()
    assert m1._handle.value is None              # freed with the case (NativeHandle: once)
    m1.close(); m1.close()
    # the library knows a handle whose case is gone: freeing it again does nothing, using it is refused by name
    assert L.lib.qgd_monitor_free(raw) == 0
    assert L.lib.qgd_monitor_sample(raw, 0) == L.ERR_INVALID and b"freed with its case" in L.lib.qgd_last_error()
    # a case freed through the device takes its monitors along as well
    case2 = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3))
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case2.set_fields(U, T, p)
    m3 = case2.monitor()
    dev.close()
    m3.close()
    case2.close()


# ---- 8. the application ----------------------------------------------------------------------------------------------------------------
def test_application_writes_what_the_monitor_reads(tmp_path):
    from qgdsolver_amd import QGDFoam
    case_dir = str(tmp_path)
    mesh = write_step_case(case_dir, "GaussVolPoint")
    locs = [(0.25, 0.5, 0.05), (2.0, 0.7, 0.05), (9.0, 9.0, 9.0)]
    with open(os.path.join(case_dir, "system", "controlDict"), "a") as f:
        f.write("functions\n{\n"
                "    wake { type probes; fields (p U rho); probeLocations (" + " ".join("(%r %r %r)" % x for x in locs) + "); writeControl timeStep; writeInterval 2; }\n"
                "    extremes { type fieldMinMax; fields (p U Mach); writeInterval 2; }\n"
                "    budget { type qgdIntegrals; writeInterval 2; }\n"
                "    ends { type qgdPatchFluxes; patches (outlet inlet); writeInterval 2; }\n"
                "    drag { type forces; patches (obstacle); }\n"
                "}\n")
    lines = []
    dev, case, _ = QGDFoam.run(case_dir, n_steps=6, write=False, log=lines.append)
    case.close(); dev.close()
    assert sum("'drag'" in x and "not served" in x for x in lines) == 1
    assert sum("probe 2 is outside the mesh" in x for x in lines) == 1

    # the same run through the API
    dev, case = ff.load_case(case_dir)
    cells = case.mesh.find_cells(locs)
    assert cells[0] >= 0 and cells[1] >= 0 and cells[2] == -1
    names = case.mesh.patch_names
    m = case.monitor(probes=cells, patches=[names.index("outlet"), names.index("inlet")])
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

    for name, cols in (("p", [4]), ("rho", [0]), ("U", [1, 2, 3])):
        text = open(os.path.join(post, "wake", "0", name)).read().splitlines()
        assert text[2].endswith("# Not Found") and text[4] == "# Time"
        rows = np.array([[float(x) for x in ln.replace("(", " ").replace(")", " ").split()] for ln in text if not ln.startswith("#")])
        assert rows.shape == (3, 1 + 3 * len(cols))
        for r, s in zip(rows, want):
            assert r[0] == s["time"] and np.array_equal(r[1:], s["probes"][:, cols].reshape(-1), equal_nan=True)
    rows = table("budget", "0", "volIntegrals.dat")
    assert rows.shape == (3, 11)
    for r, s in zip(rows, want):
        assert r[0] == s["time"] and np.array_equal(r[1:9], s["integrals"]) and r[9] == 0 and r[10] == -1
    rows = table("extremes", "0", "fieldMinMax.dat")
    assert rows.shape == (3, 31)
    for r, s in zip(rows, want):
        for j, k in enumerate((1, 3, 4)):
            blk = r[1 + 10 * j:11 + 10 * j]
            assert blk[0] == s["min"][k] and blk[1] == s["minCell"][k] and np.array_equal(blk[2:5], C[s["minCell"][k]])
            assert blk[5] == s["max"][k] and blk[6] == s["maxCell"][k] and np.array_equal(blk[7:10], C[s["maxCell"][k]])
    rows = table("ends", "0", "patchFluxes.dat")
    assert rows.shape == (3, 19)
    for r, s in zip(rows, want):
        assert r[0] == s["time"]
        for j in range(2):
            blk = r[1 + 9 * j:10 + 9 * j]
            assert blk[0] == s["patchArea"][j] and np.array_equal(blk[1:6], s["patchFlux"][j]) and np.array_equal(blk[6:9], s["patchPressureForce"][j])
    assert np.abs(rows[:, 2]).min() > 0          # mass leaves through the outlet
