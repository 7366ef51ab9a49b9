"""Run monitor of a resident QHDFoam / SRFQHDFoam case (qgd_qhd_monitor_create, qgdsolver_amd/csrc/qgd_qhd_monitor.hip): integrals,
the continuity error of the pressure solve, extrema, probes and patch totals against numpy on the case's own fields, the discrete
balances of U and T they close, shards, non-interference, refusals and the two applications.

Bounds.  A sum of n terms is compared with math.fsum of the terms under n * 2^-52 * sum |term| (test_monitor_gpu.sum_ok's rule: it holds
for every order of summation).  Where a term is itself formed by r rounded operations (U_k V: 1; |U|^2/2 V: 6; beta T g_k V: 3) numpy and
the device may round it differently (other order, fused multiply-add), by at most r * 2^-52 of its magnitude, so n becomes n + r.
Extrema, labels and probe values of stored fields are compared exactly; |U| (six rounded operations) to 6 * 2^-52 relative.
d_c, the signed sum of phi over the nf_c faces of cell c, is rebuilt in numpy from phi, owner and neighbour: the device's d_c and
numpy's differ by at most pc_c = nf_c * 2^-52 * sum_f |phi_f| (two sums of nf_c terms in different orders)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd import foamfile as ff
from qgdsolver_amd import qhdfoam
from qgdsolver_amd.halo import LocalWorld, QhdStepper
from qgdsolver_amd.monitor import QHDMonitor, combine, continuity_errors

import srf_ref as R
from qhd_shards import range_shards
from test_qhd_case import cavity_bcs, initial, options
from test_qhdfoam_case import write_cavity_case
from util import make_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def sum_ok(got, terms, what, n=None, mags=None):
    """|got - fsum(terms)| <= n * 2^-52 * fsum(|terms|) (mags: the magnitudes that enter the bound where a term is a difference)"""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    n = terms.size if n is None else n
    exact = math.fsum(terms)
    bound = n * EPS * math.fsum(np.abs(terms) if mags is None else np.asarray(mags).reshape(-1))
    print(f"{what}: got {got!r} exact {exact!r} |diff| {abs(got - exact):.3e} bound {bound:.3e}")
    assert abs(got - exact) <= bound, (what, got, exact, abs(got - exact), bound)


def perturbed(mesh, seed=3, amp=1e-2):
    U, T, p = initial(mesh)
    U = U + amp * np.random.default_rng(seed).standard_normal(U.shape)
    if mesh.nGeometricD == 2:
        U[:, 2] = 0.0
    return U, T, p


def open_case(mesh, fields=None, srf=None, solve_T=False, **opt):
    dev = q.Device(mesh)
    case = qhdfoam.QHDFoamCase(dev, options("GaussVolPoint" if mesh.nGeometricD == 3 else "leastSquares", **dict(dict(deltaT=1e-3), **opt)))
    if srf is not None:
        case.set_srf(srf, solve_T=solve_T)
    cavity_bcs(case, mesh)
    case.set_fields(*(fields if fields is not None else perturbed(mesh)))
    return dev, case


def cell_divergence(mesh, phi):
    """(d_c, sum_f |phi_f| per cell, faces per cell) from phi, owner and neighbour"""
    own, nei, nif = mesh.array("owner"), mesh.array("neighbour"), mesh.nInternalFaces
    d, a = np.zeros(mesh.nCells), np.zeros(mesh.nCells)
    np.add.at(d, own, phi)
    np.subtract.at(d, nei, phi[:nif])
    np.add.at(a, own, np.abs(phi))
    np.add.at(a, nei, np.abs(phi[:nif]))
    nf = np.bincount(own, minlength=mesh.nCells) + np.bincount(nei, minlength=mesh.nCells)
    return d, a, nf


def body_force(case, U, T, omega=None):
    """(B, magnitudes of its parts) per cell as the cell update forms it: beta T g - 2 omega ^ U"""
    o = case.options
    g = np.array([o.g[0], o.g[1], o.g[2]])
    B = (o.beta * T)[:, None] * g[None, :]
    mag = np.abs(B)
    if omega is not None:
        w = np.asarray(omega, dtype=np.float64)
        B = B - 2.0 * np.cross(w, U)
        mag = mag + 2.0 * np.stack([np.abs(w[1] * U[:, 2]) + np.abs(w[2] * U[:, 1]), np.abs(w[2] * U[:, 0]) + np.abs(w[0] * U[:, 2]),
                                    np.abs(w[0] * U[:, 1]) + np.abs(w[1] * U[:, 0])], axis=1)
    return B, mag


def check_cells(s, case, mesh, owned=None, labels=None, what="", omega=None):
    """integrals, continuity entries and extrema of a sample against numpy over the owned cells of the case's fields"""
    V_all = mesh.array("V")
    owned = np.arange(V_all.size) if owned is None else owned
    labels = owned if labels is None else labels
    U, T, p, V = case.field("U")[owned], case.field("T")[owned], case.field("p")[owned], V_all[owned]
    n = owned.size
    assert s["ownedCells"] == n and s["nonFinite"] == 0 and s["firstNonFinite"] == -1
    u2 = U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1] + U[:, 2] * U[:, 2]
    sum_ok(s["volume"], V, what + " volume")
    for k in range(3):
        sum_ok(s["momentum"][k], U[:, k] * V, what + f" U{k} V", n=n + 1)
    sum_ok(s["integrals"][4], T * V, what + " T V", n=n + 1)
    sum_ok(s["integrals"][5], 0.5 * u2 * V, what + " kinetic", n=n + 6)
    sum_ok(s["integrals"][6], p * V, what + " p V", n=n + 1)
    B, mag = body_force(case, U, T, omega)
    for k in range(3):
        sum_ok(s["bodyForce"][k], B[:, k] * V, what + f" B{k} V", n=n + (3 if omega is None else 7), mags=mag[:, k] * V)
    rows = [("magU", np.sqrt(u2), 6 * EPS), ("T", T, 0.0), ("p", p, 0.0)]
    if s["fluxState"] == 0:
        assert np.isnan(s["continuityGlobal"]) and np.isnan(s["continuityLocal"]) and np.isnan(s["min"][3]) and np.isnan(s["max"][3])
        assert s["minCell"][3] == -1 and s["maxCell"][3] == -1
    else:
        phi = case.field("phi")
        d, a, nf = cell_divergence(mesh, phi)
        d, pc = d[owned], (nf * EPS * a)[owned]
        if owned.size == V_all.size:      # all signed terms: every face for its owner, the internal ones for their neighbour
            terms = np.concatenate([phi, -phi[:mesh.nInternalFaces]])
            sum_ok(s["continuityGlobal"], terms, what + " sum d_c")
        else:                             # a shard: its owned cells' d_c, each within pc_c of numpy's, then a sum of n terms
            exact, bound = math.fsum(d), math.fsum(pc) + n * EPS * math.fsum(np.abs(d))
            print(f"{what} sum d_c (owned): got {s['continuityGlobal']!r} numpy {exact!r} |diff| {abs(s['continuityGlobal'] - exact):.3e} bound {bound:.3e}")
            assert abs(s["continuityGlobal"] - exact) <= bound, (what, s["continuityGlobal"], exact, bound)
        exact = math.fsum(np.abs(d))
        bound = math.fsum(pc) + n * EPS * exact
        print(f"{what} sum |d_c|: got {s['continuityLocal']!r} numpy {exact!r} |diff| {abs(s['continuityLocal'] - exact):.3e} bound {bound:.3e}")
        assert abs(s["continuityLocal"] - exact) <= bound, (what, s["continuityLocal"], exact, bound)
        # the continuity extremum: within the per-cell part of that bound, and the cell named holds a value within it
        r, tol = np.abs(d) / V, pc / V + EPS * np.abs(d) / V
        for val, cell, best in (("min", "minCell", np.min(r + tol)), ("max", "maxCell", np.max(r - tol))):
            got, at = s[val][3], int(s[cell][3])
            j = int(np.nonzero(labels == at)[0][0])
            print(f"{what} {val} contErr: got {got!r} at {at}, numpy there {r[j]!r} +- {tol[j]:.3e}")
            assert abs(got - r[j]) <= tol[j], (what, val, got, r[j], tol[j])
            assert (r[j] - tol[j] <= best) if val == "min" else (r[j] + tol[j] >= best), (what, val, at, r[j], best)
    for k, (name, a, rtol) in enumerate(rows):
        for val, cell, arg in (("min", "minCell", np.argmin), ("max", "maxCell", np.argmax)):
            i = int(arg(a))                       # numpy's first occurrence: the lowest label of a tie (labels ascend with position)
            got, at = s[val][k], int(s[cell][k])
            print(f"{what} {val} {name}: got {got!r} at {at}, numpy {a[i]!r} at {labels[i]}")
            if rtol == 0.0:
                assert got == a[i] and at == labels[i], (what, val, name, got, a[i], at, labels[i])
            else:
                assert abs(got - a[i]) <= rtol * abs(a[i]), (what, val, name, got, a[i])
                j = int(np.nonzero(labels == at)[0][0])      # the cell named holds that value (a rounding may move a near-tie)
                assert abs(a[j] - a[i]) <= rtol * abs(a[i]), (what, val, name, at, labels[i])


def check_probes(s, case, cells):
    U, T, p = case.field("U"), case.field("T"), case.field("p")
    for row, c in zip(s["probes"], cells):
        if c < 0:
            assert np.isnan(row).all()
            continue
        assert np.array_equal(row[0:3], U[c]) and row[3] == T[c] and row[4] == p[c]


def check_continuity_closes(s, case, mesh, what=""):
    """with all real patches requested: sum_c d_c equals the patches' volumetric fluxes within (nCells + nFaces) 2^-52 sum |phi|"""
    bound = (mesh.nCells + mesh.nFaces) * EPS * math.fsum(np.abs(case.field("phi")))
    through = math.fsum(s["patchFlux"][:, 0])
    print(f"{what} continuity closes: sum d_c {s['continuityGlobal']!r} through the patches {through!r} |diff| {abs(s['continuityGlobal'] - through):.3e} bound {bound:.3e}")
    assert np.isfinite(s["continuityGlobal"]) and abs(s["continuityGlobal"] - through) <= bound, (what, s["continuityGlobal"], through, bound)


# ---- 1. layout ---------------------------------------------------------------------------------------------------------------------------
def test_layout_and_grid_cap():
    dev, case = open_case(q.PolyMesh.box(2, 2, 2))
    m = case.monitor(probes=[0, 7, -1], patches=[0, 5])
    assert isinstance(m, QHDMonitor)
    assert m.offsets == [0, 8, 20, 36, 51] and m.n_doubles == 51 + 18 and m.grid_cap == 1024 and L.ABI_VERSION == 9
    case.close(); dev.close()


# ---- 2. against numpy on case.field() ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box111", "box5_3_17", "box488", "box257_1_1", "box654_poly", "tet433", "prism543", "mix643", "box64_64_65", "ref533"])
def test_integrals_extrema_and_probes_against_numpy(kind):
    dims = {"box111": (1, 1, 1), "box5_3_17": (5, 3, 17), "box488": (4, 8, 8), "box257_1_1": (257, 1, 1), "box64_64_65": (64, 64, 65)}
    mesh = make_mesh(kind) if kind not in dims else q.PolyMesh.box(*dims[kind])
    assert {"box5_3_17": 255, "box488": 256, "box257_1_1": 257}.get(kind, mesh.nCells) == mesh.nCells
    if kind in ("tet433", "prism543"):           # the cell-face walk on cells of four and five faces
        nf = np.bincount(mesh.array("owner"), minlength=mesh.nCells) + np.bincount(mesh.array("neighbour"), minlength=mesh.nCells)
        assert set(nf) == ({4} if kind == "tet433" else {5})
    dev, case = open_case(mesh, pTol=1e-10 if kind == "box64_64_65" else 1e-12)
    probes = sorted({0, mesh.nCells // 2, mesh.nCells - 1}) + [-1]
    m = case.monitor(probes=probes)
    steps = 3
    if kind == "box64_64_65":
        assert mesh.nCells > m.grid_cap * 256       # lanes take a second trip
        steps = 1
    case.step(steps)
    m.sample()
    s = m.read()
    assert s["step"] == steps and s["time"] == case.info()["time"] and s["deltaT"] == 1e-3 and s["fluxState"] == 1
    assert not s["rotating"] and not s["frozenT"]
    check_cells(s, case, mesh, what=kind)
    check_probes(s, case, probes)
    case.close(); dev.close()


# ---- 3. special values ---------------------------------------------------------------------------------------------------------------------
def test_uniform_state_puts_every_extremum_at_the_first_owned_cell():
    mesh = q.PolyMesh.box(9, 8, 7)
    n = mesh.nCells
    dev, case = open_case(mesh, fields=(np.tile([0.1, 0.2, 0.3], (n, 1)), np.full(n, 301.0), np.full(n, 0.9)))
    m = case.monitor()
    m.sample()
    s = m.read()
    assert np.array_equal(s["minCell"][:3], np.zeros(3)) and np.array_equal(s["maxCell"][:3], np.zeros(3)), (s["minCell"], s["maxCell"])
    assert np.array_equal(s["min"][:3], s["max"][:3]) and s["min"][1] == 301.0 and s["min"][2] == 0.9
    assert s["fluxState"] == 0 and s["minCell"][3] == -1 and s["maxCell"][3] == -1 and np.isnan(s["min"][3]) and np.isnan(s["max"][3])
    case.close(); dev.close()
    # a shard: the first owned cell is not local cell 0, and its label is that of the unsharded mesh
    sh = mesh.shard(3, 1)
    cg = sh.array("cellGlobal")
    dev, case = open_case(sh, fields=(np.tile([0.1, 0.2, 0.3], (cg.size, 1)), np.full(cg.size, 301.0), np.full(cg.size, 0.9)))
    m = case.monitor()
    m.sample()
    s = m.read()
    first = n // 3
    assert first in cg and cg[0] < first
    assert np.array_equal(s["minCell"][:3], np.full(3, first)) and np.array_equal(s["maxCell"][:3], np.full(3, first)), (s["minCell"], first)
    assert s["ownedCells"] == (2 * n) // 3 - n // 3
    case.close(); dev.close()


def test_one_nan_cell_is_counted_named_and_kept_out_of_the_extrema():
    mesh = q.PolyMesh.box(7, 6, 5)
    U, T, p = perturbed(mesh)
    p = 0.1 * np.random.default_rng(5).standard_normal(mesh.nCells)
    bad = 137
    T = T.copy()
    T[bad] = np.nan
    dev, case = open_case(mesh, fields=(U, T, p))
    m = case.monitor(patches=range(6))
    m.sample()                                   # no step taken
    s = m.read()
    assert s["nonFinite"] == 1 and s["firstNonFinite"] == bad
    # before the first step: flux state 0, the patch fluxes and the continuity entries are NaN; areas and pressure forces are not
    assert s["fluxState"] == 0 and np.isnan(s["patchFlux"]).all() and np.isnan(s["continuityGlobal"]) and np.isnan(s["continuityLocal"])
    assert np.isfinite(s["patchArea"]).all() and np.isfinite(s["patchPressureForce"]).all()
    others = np.delete(np.arange(mesh.nCells), bad)
    Tt, pp = case.field("T")[others], case.field("p")[others]
    assert s["min"][1] == Tt.min() and s["minCell"][1] == others[np.argmin(Tt)] and s["max"][1] == Tt.max() and s["maxCell"][1] == others[np.argmax(Tt)]
    assert s["min"][2] == pp.min() and s["minCell"][2] == others[np.argmin(pp)] and s["max"][2] == pp.max() and s["maxCell"][2] == others[np.argmax(pp)]
    assert bad not in s["minCell"] and bad not in s["maxCell"] and np.isfinite(s["min"][:3]).all() and np.isfinite(s["max"][:3]).all()
    # the sums that meet the cell are NaN; the others are not
    assert np.isnan(s["integrals"][4]) and np.isnan(s["bodyForce"][1])
    sum_ok(s["volume"], mesh.array("V"), "volume next to a NaN cell")
    sum_ok(s["integrals"][6], case.field("p") * mesh.array("V"), "p V next to a NaN cell", n=mesh.nCells + 1)
    case.close(); dev.close()


# ---- 4. patch totals against the face fields, 5. continuity closes ------------------------------------------------------------------------
def check_patches(s, case, mesh, patches, faces_of=None, what=""):
    ps, pz = mesh.array("patchStart"), mesh.array("patchSize")
    phi, F = case.field("phi"), case.field("faceTerms")
    Sf, mag = mesh.array("Sf").reshape(-1, 3), mesh.array("magSf")
    pb = case.field("p.boundary")
    nif = mesh.nInternalFaces
    terms = {}
    for row, pa in enumerate(patches):
        f = np.arange(ps[pa], ps[pa] + pz[pa]) if faces_of is None else faces_of(pa)
        tag = f"{what} patch {pa} ({f.size} faces)"
        sum_ok(s["patchArea"][row], mag[f], tag + " area")
        sum_ok(s["patchFlux"][row, 0], phi[f], tag + " phi")
        for k in range(4):
            if k == 3 and s["frozenT"]:
                assert np.isnan(s["patchFlux"][row, 4])
                continue
            sum_ok(s["patchFlux"][row, 1 + k], F[k][f], tag + f" face term {k}")
        for k in range(3):
            sum_ok(s["patchPressureForce"][row, k], pb[f - nif] * Sf[f, k], tag + f" p Sf {k}", n=f.size + 1)
        terms[pa] = f
    return terms


@pytest.mark.parametrize("kind", ["box111", "box20_17_3", "box654_poly", "box257_257_1", "tet433", "ref533"])
def test_patch_totals_against_the_face_fields(kind):
    dims = {"box111": (1, 1, 1), "box20_17_3": (20, 17, 3), "box257_257_1": (257, 257, 1)}
    mesh = q.PolyMesh.box(*dims[kind]) if kind in dims else make_mesh(kind)
    # (the totals are compared with the face fields of the same state, converged or not: the large mesh opens with a loose pressure tolerance)
    dev, case = open_case(mesh, **(dict(pTol=1e-6) if kind == "box257_257_1" else {}))
    patches = [5, 0, 1, 2, 3, 4, 0]                  # any order, one of them twice
    m = case.monitor(patches=patches)
    with pytest.raises(q.QgdError, match="before the first step"):
        case.field("faceTerms")
    case.step(2)
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
    assert np.abs(case.field("faceTerms")[:, mesh.nInternalFaces:]).max() > 0
    # 5: with every real patch once, the global continuity error is what leaves through the patches
    m6 = case.monitor(patches=range(6))
    m6.sample()
    check_continuity_closes(m6.read(), case, mesh, what=kind)
    case.close(); dev.close()


# ---- 6. balances ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["plain", "rotating", "rotating_solve_T"])
def test_patch_totals_close_the_balances_of_momentum_and_temperature(arm):
    """after each of 5 explicit steps, for k = x, y, z:
    |sum U_k V (n) - sum U_k V (n-1) + dt sum F_k (n) - dt bodyForce_k (n-1)| <= (nCells + nFaces) 2^-52 (sum |U_k V| + dt sum_boundary |F_k| + dt sum |B_k V|),
    the same for T without the source; with T frozen sum T V is bitwise constant and the T flux column is NaN"""
    mesh = q.PolyMesh.box(10, 9, 8)
    omega = None if arm == "plain" else R.OMEGA_3D
    dev, case = open_case(mesh, srf=omega, solve_T=arm == "rotating_solve_T", fields=perturbed(mesh, amp=5e-2))
    frozen = arm == "rotating"
    m = case.monitor(patches=range(6))
    V = mesh.array("V")
    nif = mesh.nInternalFaces
    dt = 1e-3
    m.sample()
    prev = m.read()
    assert prev["rotating"] == (omega is not None) and prev["frozenT"] == frozen
    big = (mesh.nCells + mesh.nFaces) * EPS
    for step in range(1, 6):
        U0, T0 = case.field("U"), case.field("T")
        B, mag = body_force(case, U0, T0, omega)
        for k in range(3):                           # the body force of the state the step starts from, as the step will form it
            sum_ok(prev["bodyForce"][k], B[:, k] * V, f"{arm} step {step} B{k} V", n=mesh.nCells + (3 if omega is None else 7), mags=mag[:, k] * V)
        case.step(1)
        m.sample()
        s = m.read()
        assert s["fluxState"] == 1 and s["step"] == step and s["deltaT"] == dt
        U, T, F = case.field("U"), case.field("T"), case.field("faceTerms")
        Fsum = s["patchFlux"].sum(axis=0)            # volumetric, U x 3, T over all patches
        for k, name in enumerate(("Ux", "Uy", "Uz")):
            absF = math.fsum(np.abs(F[k][nif:]))
            assert absF > 0 and abs(Fsum[1 + k]) > 0 and np.abs(s["patchFlux"][:, 1 + k]).sum() > 0     # the test cannot pass on zeros
            defect = abs(s["momentum"][k] - prev["momentum"][k] + dt * Fsum[1 + k] - dt * prev["bodyForce"][k])
            bound = big * (math.fsum(np.abs(U[:, k] * V)) + dt * absF + dt * math.fsum(np.abs(B[:, k] * V)))
            print(f"{arm} step {step} {name}: dQ {s['momentum'][k] - prev['momentum'][k]:.6e} dt*F {dt * Fsum[1 + k]:.6e} dt*B {dt * prev['bodyForce'][k]:.6e} "
                  f"defect {defect:.3e} bound {bound:.3e}")
            assert defect <= bound, (arm, step, name, defect, bound)
        if frozen:
            assert s["integrals"][4] == prev["integrals"][4] and np.isnan(s["patchFlux"][:, 4]).all() and np.array_equal(T, T0)
        else:
            absF = math.fsum(np.abs(F[3][nif:]))
            assert absF > 0 and abs(Fsum[4]) > 0
            defect = abs(s["integrals"][4] - prev["integrals"][4] + dt * Fsum[4])
            bound = big * (math.fsum(np.abs(T * V)) + dt * absF)
            print(f"{arm} step {step} T: dQ {s['integrals'][4] - prev['integrals'][4]:.6e} dt*F {dt * Fsum[4]:.6e} defect {defect:.3e} bound {bound:.3e}")
            assert defect <= bound, (arm, step, "T", defect, bound)
        check_continuity_closes(s, case, mesh, what=f"{arm} step {step}")
        prev = s
    case.close(); dev.close()


# ---- 7. implicitDiffusion ------------------------------------------------------------------------------------------------------------------
def test_implicit_diffusion_reports_the_volumetric_flux_and_the_continuity_errors_only():
    mesh = q.PolyMesh.box(6, 5, 4)
    dev, case = open_case(mesh, implicitDiffusion=1, implicitTol=1e-12, implicitMaxIter=2000)
    m = case.monitor(patches=range(6))
    case.step(2)
    m.sample()
    s = m.read()
    assert s["fluxState"] == 2 and np.isfinite(s["patchFlux"][:, 0]).all() and np.isnan(s["patchFlux"][:, 1:]).all()
    assert np.isfinite(s["patchArea"]).all() and np.isfinite(s["continuityLocal"]) and np.isfinite(s["min"][3]) and np.isfinite(s["max"][3])
    check_continuity_closes(s, case, mesh, what="implicitDiffusion")
    check_cells(s, case, mesh, what="implicitDiffusion")
    case.close(); dev.close()


# ---- 8. shards -----------------------------------------------------------------------------------------------------------------------------
def test_three_shards_on_one_device_add_up_to_the_unsharded_monitor():
    g = make_mesh("box654_poly")
    g.renumber(np.random.default_rng(4).permutation(g.nCells).astype(np.int32))
    g.renumber(g.morton_order())
    n = g.nCells
    fields = perturbed(g)
    patches, probe_cells = list(range(6)), [5, 60, 110]
    gdev, whole = open_case(g, fields=fields, pRefCell=111, pRefValue=0.25)
    mon = whole.monitor(patches=patches, probes=probe_cells)
    mon.sample()
    before = mon.read()                              # the state both runs start from
    shards = range_shards(g, 3)
    keep, mons = [], []
    for sh in shards:
        cg = sh["cell_global"]
        d, c = open_case(sh["mesh"], fields=tuple(f[cg] for f in fields), pRefCell=111, pRefValue=0.25)
        with pytest.raises(q.QgdError, match="halo patch") as ei:
            c.monitor(patches=[sh["mesh"].nPatches - 1])
        assert ei.value.code == L.ERR_INVALID
        where = {int(cg[i]): int(i) for i in sh["owned"]}
        mons.append(c.monitor(patches=patches, probes=[where.get(x, -1) for x in probe_cells]))
        keep.append((d, c))
    cases = [c for _, c in keep]

    def sample_all():
        parts = []
        for sh, c, mo in zip(shards, cases, mons):
            mo.sample()
            s = mo.read()
            assert s["ownedCells"] == sh["owned"].size < sh["mesh"].nCells
            s.pop("raw")
            parts.append(s)
        return parts

    # the same state: sums within the bound of the combined terms, extrema, their cells and the probes equal
    tot = combine(sample_all())
    assert tot["ownedCells"] == n and tot["fluxState"] == 0 and tot["kind"] == "qhd"
    for key in ("min", "minCell", "max", "maxCell", "probes"):
        assert np.array_equal(tot[key], before[key], equal_nan=True), (key, tot[key], before[key])
    U, T, p = (whole.field(f) for f in ("U", "T", "p"))
    V = g.array("V")
    u2 = (U * U).sum(axis=1)
    Bf, mag = body_force(whole, U, T)
    cols = [(V, 0, None), (U[:, 0] * V, 1, None), (U[:, 1] * V, 1, None), (U[:, 2] * V, 1, None), (T * V, 1, None), (0.5 * u2 * V, 6, None), (p * V, 1, None)]
    cols += [(Bf[:, k] * V, 3, mag[:, k] * V) for k in range(3)]
    for k, (terms, r, mg) in enumerate(cols):
        sum_ok(tot["integrals"][k], terms, f"shards: integral {k}", n=n + 3 + r, mags=mg)
        sum_ok(before["integrals"][k], terms, f"unsharded: integral {k}", n=n + r, mags=mg)
    assert np.array_equal(tot["momentum"], tot["integrals"][1:4]) and np.array_equal(tot["bodyForce"], tot["integrals"][7:10])
    # after three steps in lockstep: every shard against its own fields over its owned cells, the combination against all their terms
    QhdStepper(LocalWorld(cases, [sh["peers"] for sh in shards])).step(3)
    parts = sample_all()
    phi_terms = {pa: [] for pa in patches}
    F_terms = {(pa, k): [] for pa in patches for k in range(4)}
    for r, (sh, c, s) in enumerate(zip(shards, cases, parts)):
        m_, own = sh["mesh"], sh["owned"]
        assert s["fluxState"] == 1 and s["step"] == 3
        check_cells(s, c, m_, owned=own, labels=sh["cell_global"][own], what=f"shard {r}")
        ps, pz, owner = m_.array("patchStart"), m_.array("patchSize"), m_.array("owner")
        is_owned = np.zeros(m_.nCells, dtype=bool)
        is_owned[own] = True

        def real_faces(pa):
            f = np.arange(ps[pa], ps[pa] + pz[pa])
            return f[is_owned[owner[f]]]
        faces = check_patches(s, c, m_, patches, faces_of=real_faces, what=f"shard {r}")
        phi, F = c.field("phi"), c.field("faceTerms")
        for pa in patches:
            phi_terms[pa].append(phi[faces[pa]])
            for k in range(4):
                F_terms[(pa, k)].append(F[k][faces[pa]])
    tot = combine(parts)
    assert tot["ownedCells"] == n and tot["fluxState"] == 1
    for row, pa in enumerate(patches):
        terms = np.concatenate(phi_terms[pa])
        assert terms.size == g.array("patchSize")[pa]            # every real face once, whoever owns it
        sum_ok(tot["patchFlux"][row, 0], terms, f"shards: patch {pa} phi", n=terms.size + 3)
        for k in range(4):
            sum_ok(tot["patchFlux"][row, 1 + k], np.concatenate(F_terms[(pa, k)]), f"shards: patch {pa} face term {k}", n=terms.size + 3)
        sum_ok(tot["patchArea"][row], g.array("magSf")[g.array("patchStart")[pa]:g.array("patchStart")[pa] + g.array("patchSize")[pa]],
               f"shards: patch {pa} area", n=terms.size + 3)
    gathered = {f: np.full((n, 3) if f == "U" else n, np.nan) for f in ("U", "T", "p")}
    for sh, c in zip(shards, cases):
        for f in gathered:
            gathered[f][sh["cell_global"][sh["owned"]]] = c.field(f)[sh["owned"]]
    for k, a in ((1, gathered["T"]), (2, gathered["p"])):
        assert tot["min"][k] == a.min() and tot["minCell"][k] == int(np.argmin(a)) and tot["max"][k] == a.max() and tot["maxCell"][k] == int(np.argmax(a))
    for row, cell in zip(tot["probes"], probe_cells):
        assert np.array_equal(row[:3], gathered["U"][cell]) and row[3] == gathered["T"][cell] and row[4] == gathered["p"][cell]
    sum_ok(tot["integrals"][4], gathered["T"] * V, "shards after 3 steps: T V", n=n + 4)
    for d, c in keep:
        c.close(); d.close()
    whole.close(); gdev.close()


# ---- 9. repeatability and the run left as it was -----------------------------------------------------------------------------------------
def test_sampling_is_repeatable_and_leaves_the_run_as_it_was():
    mesh = q.PolyMesh.box(12, 10, 8)
    dev, case = open_case(mesh)
    case.step(6)
    plain = {f: case.field(f) for f in ("U", "T", "p", "phi")}
    case.close(); dev.close()

    dev, case = open_case(mesh)
    m = case.monitor(probes=[0, 500], patches=range(6))
    rows = []
    for _ in range(6):
        case.step(1)
        m.sample()
        rows.append(m.read_raw()[0])
    for f, want in plain.items():
        assert np.array_equal(case.field(f), want), f
    a = m.read_raw(m.sample())[0]
    b = m.read_raw(m.sample())[0]
    assert a.tobytes() == b.tobytes() == rows[-1].tobytes()      # two samples of one state are bitwise equal
    assert rows[0].tobytes() != rows[1].tobytes()
    case.close(); dev.close()


def test_slots_are_read_two_samples_late():
    mesh = q.PolyMesh.box(8, 7, 6)
    dev, case = open_case(mesh)
    m = case.monitor(probes=[10])
    with pytest.raises(q.QgdError, match="never sampled"):
        m.read(2)
    with pytest.raises(q.QgdError, match="slot must be"):
        m.sample(4)
    T10, got = [], []
    for step in range(1, 9):
        case.step(1)
        T10.append(case.field("T")[10])
        assert m.sample() == (step - 1) % 4
        if step >= 3:
            got.append(m.read())                  # the oldest unread sample: two behind
            assert got[-1]["step"] == step - 2
    got += [m.read(), m.read()]
    assert [s["step"] for s in got] == list(range(1, 9))
    assert [s["probes"][0, 3] for s in got] == T10 and len(set(T10)) == 8
    with pytest.raises(ValueError):
        m.read()
    case.close(); dev.close()


# ---- 10. refusals, 11. lifetime ------------------------------------------------------------------------------------------------------------
def test_refusals_carry_their_reason():
    mesh = make_mesh("plane2d_jitter")
    dev, case = open_case(mesh)
    with pytest.raises(q.QgdError, match="empty patch") as ei:
        case.monitor(patches=[0, 4])
    assert ei.value.code == L.ERR_INVALID and "patch 4" in str(ei.value) and "qgd_qhd_monitor_create" in str(ei.value)
    with pytest.raises(q.QgdError, match="patch index 6") as ei:
        case.monitor(patches=[6])
    assert ei.value.code == L.ERR_INVALID
    for bad in (mesh.nCells, -2):
        with pytest.raises(q.QgdError, match="out of range") as ei:
            case.monitor(probes=[0, bad])
        assert ei.value.code == L.ERR_INVALID and f"cell label {bad}" in str(ei.value)
    m = case.monitor(probes=[0], patches=[0, 1, 2, 3])
    assert L.lib.qgd_monitor_enable_species(m._h) == L.ERR_INVALID and b"QHD case has no species block" in L.lib.qgd_last_error()
    with pytest.raises(q.QgdError, match="never sampled"):
        m.read(1)
    m.sample(0)
    with pytest.raises(q.QgdError, match="output too small"):
        L.check(L.lib.qgd_monitor_read(m._h, 0, np.zeros(4).ctypes.data_as(L.c_double_p), 4, None, None), "qgd_monitor_read")
    s = m.read(0)
    assert s["fluxState"] == 0 and s["ownedCells"] == mesh.nCells
    case.close(); dev.close()
    fresh = qhdfoam.QHDFoamCase(q.Device(mesh), options("leastSquares"))
    with pytest.raises(q.QgdError, match="qgd_qhd_case_set_fields first") as ei:
        fresh.monitor()
    assert ei.value.code == L.ERR_INVALID
    fresh.close(); fresh.dev.close()


def test_closing_the_case_first_frees_its_monitors_once():
    mesh = q.PolyMesh.box(4, 3, 2)
    dev, case = open_case(mesh)
    m1, m2 = case.monitor(probes=[1]), case.monitor(patches=[0])
    m3 = QHDMonitor(case, probes=[2])                # one the Python case does not know of: the library frees it with the case
    m1.sample(); m3.sample()
    raw1, raw3 = m1._handle.value, m3._handle.value
    m2.close()                                   # one closed before its case, the others after
    case.close()
    assert m1._handle.value is None              # freed with the case (NativeHandle: once)
    m1.close(); m1.close()
    # the library knows a handle whose case is gone: freeing it again does nothing, using it is refused by name
    for raw in (raw1, raw3):
        assert L.lib.qgd_monitor_free(raw) == 0
        assert L.lib.qgd_monitor_sample(raw, 0) == L.ERR_INVALID and b"freed with its case" in L.lib.qgd_last_error()
    m3.close()
    # a case freed through the device takes its monitors along as well
    case2 = qhdfoam.QHDFoamCase(dev, options("GaussVolPoint"))
    cavity_bcs(case2, mesh)
    case2.set_fields(*perturbed(mesh))
    m4 = case2.monitor()
    dev.close()
    m4.close()
    case2.close()


# ---- 12. the applications ------------------------------------------------------------------------------------------------------------------
def table(post, *path):
    return np.atleast_2d(np.loadtxt(os.path.join(post, *path), comments="#"))


def probe_rows(post, name, field):
    text = open(os.path.join(post, name, "0", field)).read().splitlines()
    return text, np.array([[float(x) for x in ln.replace("(", " ").replace(")", " ").split()] for ln in text if not ln.startswith("#")])


def check_post(case_dir, want, C, patch_count):
    post = os.path.join(case_dir, "postProcessing")
    for name, cols in (("p", [4]), ("T", [3]), ("U", [0, 1, 2])):
        text, rows = probe_rows(post, "points", name)
        assert text[2].endswith("# Not Found") and text[4] == "# Time"
        assert rows.shape == (len(want), 1 + 3 * len(cols))
        for r, s in zip(rows, want):
            assert r[0] == s["time"] and np.array_equal(r[1:], s["probes"][:, cols].reshape(-1), equal_nan=True)
    rows = table(post, "budget", "0", "volIntegrals.dat")
    assert rows.shape == (len(want), 15)
    for r, s in zip(rows, want):
        assert r[0] == s["time"] and np.array_equal(r[1:13], s["integrals"]) and r[13] == 0 and r[14] == -1
    rows = table(post, "extremes", "0", "fieldMinMax.dat")
    assert rows.shape == (len(want), 31)
    for r, s in zip(rows, want):
        for j, k in enumerate((2, 0, 3)):            # p, U (its magnitude), contErr
            blk = r[1 + 10 * j:11 + 10 * j]
            assert blk[0] == s["min"][k] and blk[1] == s["minCell"][k] and np.array_equal(blk[2:5], C[s["minCell"][k]])
            assert blk[5] == s["max"][k] and blk[6] == s["maxCell"][k] and np.array_equal(blk[7:10], C[s["maxCell"][k]])
    rows = table(post, "ends", "0", "patchFluxes.dat")
    assert rows.shape == (len(want), 1 + 9 * patch_count)
    for r, s in zip(rows, want):
        assert r[0] == s["time"]
        for j in range(patch_count):
            blk = r[1 + 9 * j:10 + 9 * j]
            assert blk[0] == s["patchArea"][j] and np.array_equal(blk[1:6], s["patchFlux"][j], equal_nan=True) and np.array_equal(blk[6:9], s["patchPressureForce"][j])
    rows = table(post, "continuity", "0", "continuityErrors.dat")
    assert rows.shape == (len(want), 6)
    cumulative = 0.0
    for r, s in zip(rows, want):
        local, glob = continuity_errors(s)
        cumulative += glob
        assert abs(local - s["deltaT"] * s["continuityLocal"] / s["volume"]) <= 2 * EPS * abs(local)      # deltaT sum |d_c| / sum V
        assert r[0] == s["time"] and r[1] == local and r[2] == glob and r[3] == cumulative and r[4] == s["max"][3] and r[5] == s["maxCell"][3]
        assert np.isfinite(local) and np.isfinite(glob) and local > 0


def functions_text(patches):
    locs = [(0.27, 0.52, 0.31), (0.81, 0.73, 0.62), (9.0, 9.0, 9.0)]
    return locs, ("functions\n{\n"
                  "    points { type probes; fields (p U T rho); probeLocations (" + " ".join("(%r %r %r)" % x for x in locs) + "); writeControl timeStep; writeInterval 2; }\n"
                  "    extremes { type fieldMinMax; fields (p U contErr); writeInterval 2; }\n"
                  "    budget { type qhdIntegrals; writeInterval 2; }\n"
                  "    ends { type qhdPatchFluxes; patches (" + " ".join(patches) + "); writeInterval 2; }\n"
                  "    continuity { type qhdContinuityErrors; writeInterval 2; }\n"
                  "    drag { type forces; patches (hot); }\n"
                  "}\n")


def load_as_the_application_does(case_dir, srf):
    """the case of <case_dir>/0 on the device, built by the calls of QHDFoam.run / SRFQHDFoam.run"""
    if srf:
        mesh, opt, fields, bcs, srf_d = ff.read_srf_case_setup(case_dir, "0")
    else:
        mesh, opt, fields, bcs = ff.read_qhd_case_setup(case_dir, "0")
    dev = q.Device(mesh, 0, fv_schemes={"fvsc": {"default": opt["stencil"]}}, fused_tables=False)
    case = qhdfoam.QHDFoamCase(dev, qhdfoam.qhd_options(**opt))
    if srf:
        case.set_srf(srf_d["omega"])
    ff.apply_qhd_bcs(case, bcs)
    case.set_fields(fields["U"], fields["T"], fields["p"])
    return dev, case


def same_time_directories(a, b, names, fields):
    for name in names:
        for f in fields:
            assert open(os.path.join(a, name, f), "rb").read() == open(os.path.join(b, name, f), "rb").read(), (name, f)


def test_qhdfoam_application_writes_what_the_monitor_reads(tmp_path):
    from qgdsolver_amd import QHDFoam
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        os.makedirs(d)
        write_cavity_case(d, implicit_line="implicitDiffusion false;")
    locs, text = functions_text(["cold", "hot"])
    with open(os.path.join(a, "system", "controlDict"), "a") as f:
        f.write(text)
    pr = subprocess.run([sys.executable, "-m", "qgdsolver_amd.QHDFoam", "-case", a], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-1500:]
    assert pr.stdout.count("'drag'") == 1 and "not served" in pr.stdout and "field 'rho' is not served" in pr.stdout
    assert pr.stdout.count("probe 2 is outside the mesh") == 1 and "max/min of T" in pr.stdout and pr.stdout.rstrip().endswith("End")
    # the run without functions{}: the same time directories, bit for bit
    dev, case, written = QHDFoam.run(b, log=lambda s: None)
    case.close(); dev.close()
    assert written == ["0.006", "0.012"]
    same_time_directories(a, b, written, ("U", "T", "p"))
    assert not os.path.exists(os.path.join(b, "postProcessing"))
    # the same run through the API
    dev, case = load_as_the_application_does(a, srf=False)
    cells = case.mesh.find_cells(locs)
    assert cells[0] >= 0 and cells[1] >= 0 and cells[2] == -1
    names = case.mesh.patch_names
    m = case.monitor(probes=cells, patches=[names.index("cold"), names.index("hot")])
    want = []
    for _ in range(6):
        case.step(2)
        m.sample()
        want.append(m.read())
    C = case.mesh.array("C").reshape(-1, 3)
    case.close(); dev.close()
    check_post(a, want, C, 2)
    assert all(s["fluxState"] == 1 and not s["rotating"] for s in want)


def test_srfqhdfoam_application_writes_what_the_monitor_reads(tmp_path):
    from qgdsolver_amd import SRFQHDFoam
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        os.makedirs(d)
        R.write_srf_case(d)
    locs, text = functions_text(["casing", "rotor", "floor"])
    with open(os.path.join(a, "system", "controlDict"), "a") as f:
        f.write(text.replace("patches (hot)", "patches (rotor)"))
    pr = subprocess.run([sys.executable, "-m", "qgdsolver_amd.SRFQHDFoam", "-case", a], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-1500:]
    assert pr.stdout.count("'drag'") == 1 and "not served" in pr.stdout and pr.stdout.rstrip().endswith("End")
    dev, case, written = SRFQHDFoam.run(b, log=lambda s: None)
    case.close(); dev.close()
    assert written == ["0.003", "0.006"]
    same_time_directories(a, b, written, ("Urel", "Uabs", "T", "p"))
    dev, case = load_as_the_application_does(a, srf=True)
    cells = case.mesh.find_cells(locs)
    names = case.mesh.patch_names
    m = case.monitor(probes=cells, patches=[names.index(p) for p in ("casing", "rotor", "floor")])
    want = []
    for _ in range(3):
        case.step(2)
        m.sample()
        want.append(m.read())
    C = case.mesh.array("C").reshape(-1, 3)
    case.close(); dev.close()
    assert all(s["rotating"] and s["frozenT"] and np.isnan(s["patchFlux"][:, 4]).all() and np.isfinite(s["patchFlux"][:, :4]).all() for s in want)
    check_post(a, want, C, 3)
