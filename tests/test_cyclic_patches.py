"""Translational cyclic patch pairs served by ghost cells (qgd_mesh_unroll_cyclic): the two halves of a pair are glued -- behind
each half sit translated copies of the cells that touch the other half, refreshed from their originals once per step by the halo pack / unpack of
the same rank.  What is checked, with properties a shared mistake of oracle and device could not satisfy:
  * the extended mesh is consistent (every real cell / point / patch face keeps its label, the cyclic patches are empty, the copies of the two
    sides of a pair mirror each other);
  * a box periodic in x reproduces, cell for cell, the middle third of the SAME case on a three times longer box without any cyclic patch
    (information travels a few cells per step: for the first steps the middle third cannot know the long box ends);
  * a triply periodic box conserves mass, momentum and total energy to rounding (edge and corner copies included);
  * a pulse carried by a uniform flow leaves through one half and re-enters through the other;
  * rotational or unmatched halves are refused by name;
and, on the GPU, the device case -- plain qgd_case_step, the library refreshes the copies itself -- against the oracle driven by hand, through the
fused one-launch step and through the separate kernels."""
import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L

import cases
from oracle import OracleCase, OracleMesh

G, CYC = L.PATCH_GENERIC, L.PATCH_CYCLIC


def periodic_box(n, periodic=(True, False, False), lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), jitter=0.0, seed=2024):
    """jitter: the interior points are moved by up to jitter * h (PolyMesh.jitter keeps every boundary point where it is, so the two halves
    of a pair still match point by point: a legal periodic case whose cells are no translates of each other)"""
    pt = []
    for d in range(3):
        pt += [CYC, CYC] if periodic[d] else [G, G]
    mesh = q.PolyMesh.box(n[0], n[1], n[2], lo=lo, hi=hi, patch_types=pt)
    if jitter:
        mesh.jitter(jitter, seed=seed)
    return mesh


class OraclePeriodic:
    """the oracle on an unrolled mesh, its copies refreshed by hand: pack every slot, unpack what the partner slot packed"""

    def __init__(self, ext, options, bc_fn=None):
        self.ext = ext
        om = OracleMesh(ext.primitives())
        self.self_slot = [int(x) for x in ext.array("haloSelf")]
        for k in range(ext.halo_slots):
            om.set_halo(k, ext.array(f"haloGhost{k}"), ext.array(f"haloSend{k}"))
        om.set_halo_face_h(ext.array("haloFaceH"))
        self.case = OracleCase(om, options)
        if bc_fn:
            bc_fn(self.case)

    def exchange(self, mid=False):
        c = self.case
        bufs = []
        for k in range(len(self.self_slot)):
            if mid:
                b = np.zeros(c.mid_halo_count(k)[0]); c.mid_halo_pack(k, b)
            else:
                b = np.zeros(c.halo_count(k)); c.halo_pack(k, b)
            bufs.append(b)
        for k, src in enumerate(self.self_slot):
            if mid:
                assert bufs[src].size == c.mid_halo_count(k)[1]
                c.mid_halo_unpack(k, bufs[src])
            else:
                assert bufs[src].size == c.halo_recv_count(k)
                c.halo_unpack(k, bufs[src])
        if not mid:
            c.step_phase(2)

    def set_fields(self, U, T, p):
        cg = self.ext.array("cellGlobal")
        self.case.set_fields(U[cg], T[cg], p[cg])
        self.exchange()

    def step(self, n):
        c = self.case
        for _ in range(n):
            if c.needs_mid_exchange():
                c.step_phase(5); self.exchange(mid=True); c.step_phase(6)
            else:
                c.step_phase(0)
            c.step_phase(1)
            self.exchange()

    def update_fluxes(self):
        """the flux assembly on current copies, with the message in the middle of it where a step has one (a qgdFlux wall under GaussVolPoint)"""
        c = self.case
        if c.needs_mid_exchange():
            c.step_phase(5); self.exchange(mid=True); c.step_phase(6)
        else:
            c.updateFluxes()

    def field(self, name, n_real):
        return self.case.field(name)[:n_real]


def test_unrolled_mesh_keeps_the_real_mesh_and_mirrors_its_sides():
    g = periodic_box((6, 5, 4), (True, True, False))
    ext = g.unroll_cyclic()
    n = g.nCells
    assert ext.nCells > n and np.array_equal(ext.array("cellGlobal")[:n], np.arange(n))
    assert np.array_equal(ext.array("points")[:3 * g.nPoints], g.array("points"))
    ps, pz, pty = ext.array("patchStart"), ext.array("patchSize"), ext.array("patchType")
    assert ext.nPatches == g.nPatches + 1 and pty[-1] == L.PATCH_HALO and pz[-1] > 0
    assert all(pz[i] == 0 for i in range(g.nPatches) if pty[i] == CYC)
    # a box periodic in x and y: 8 tiles have copies (4 sides + 4 edges), each slot's ghosts are its partner's send list shifted
    self_slot = ext.array("haloSelf")
    assert ext.halo_slots == 8 and sorted(self_slot) == list(range(8)) and all(self_slot[self_slot[k]] == k for k in range(8))
    cg = ext.array("cellGlobal")
    C = ext.array("C").reshape(-1, 3)
    for k in range(8):
        ghost, send = ext.array(f"haloGhost{k}"), ext.array(f"haloSend{int(self_slot[k])}")
        assert np.array_equal(cg[ghost], send)               # the copies are exactly the cells the partner slot sends, in its order
        shift = C[ghost] - C[send]
        assert np.abs(shift - shift[0]).max() < 1e-12 and np.abs(shift[0]).max() > 0.5       # ... all shifted by ONE lattice vector
    # every cyclic face of the real mesh became an internal face: nothing of the real cells is left on the halo patch
    own = ext.array("owner")
    assert (own[ps[-1]: ps[-1] + pz[-1]] >= n).all()
    # the zMin / zMax patches got the copies' faces behind the real ones, which kept their order
    fg = ext.array("faceGlobal")
    for i in (4, 5):
        real = fg[ps[i]: ps[i] + g.array("patchSize")[i]]
        assert np.array_equal(real, np.arange(g.array("patchStart")[i], g.array("patchStart")[i] + g.array("patchSize")[i]))
        assert pz[i] > g.array("patchSize")[i]


def test_rotational_or_unmatched_halves_are_refused_by_name():
    g = periodic_box((4, 4, 4), (True, False, False))
    with pytest.raises(q.QgdError, match="not both cyclic"):
        g.unroll_cyclic([(0, 2)])
    h = q.PolyMesh.box(4, 4, 4, patch_types=[CYC, G, CYC, G, G, G])       # xMin paired with yMin: not translates of each other
    with pytest.raises(q.QgdError, match="not translates"):
        h.unroll_cyclic([(0, 2)])
    plain = q.PolyMesh.box(4, 4, 4)
    with pytest.raises(q.QgdError, match="no cyclic patches"):
        plain.unroll_cyclic()


def tiled_fields(fields_fn, C, period):
    """fields of the periodic case evaluated on any box: x taken modulo the period"""
    Cm = C.copy()
    Cm[:, 0] = np.mod(Cm[:, 0], period)
    return fields_fn(Cm)


def smooth_fields(C):
    x, y, z = C[:, 0], C[:, 1], C[:, 2]
    U = np.stack([0.3 + 0.1 * np.sin(2 * np.pi * x) * np.cos(np.pi * y), 0.05 * np.cos(2 * np.pi * x) * np.sin(np.pi * y),
                  0.02 * np.sin(4 * np.pi * x) * np.sin(np.pi * z)], axis=1)
    T = 1.0 + 0.05 * np.cos(2 * np.pi * x) * np.cos(np.pi * y)
    p = 1.0 + 0.1 * np.sin(2 * np.pi * x + 0.3) * np.cos(np.pi * z)
    return U, T, p


def wall_bcs(case):
    """slip walls with the qgdFlux pressure condition on y, zeroGradient on z (patches 2..5; 0, 1 are the cyclic halves)"""
    for patch in (2, 3):
        case.set_bc(patch, U=("slip", None), T=("zeroGradient", None), p=("qgdFlux", None))


@pytest.mark.parametrize("stencil,bc_fn", [("GaussVolPoint", None), ("GaussVolPoint", wall_bcs), ("reduced", None)])
def test_periodic_box_is_the_middle_of_a_three_times_longer_box(stencil, bc_fn):
    nx, ny, nz, steps = 8, 5, 4, 3
    opt = q.default_options(stencil=stencil, deltaT=2e-3, mu=1e-3)
    g = periodic_box((nx, ny, nz), (True, False, False))
    ext = g.unroll_cyclic()
    per = OraclePeriodic(ext, opt, bc_fn)
    per.set_fields(*smooth_fields(g.array("C").reshape(-1, 3)))
    per.step(steps)
    # the same case on [-1, 2) x [0, 1)^2 with ordinary patches at its far ends
    long = q.PolyMesh.box(3 * nx, ny, nz, lo=(-1.0, 0.0, 0.0), hi=(2.0, 1.0, 1.0))
    oc = OracleCase(OracleMesh(long.primitives()), opt)
    if bc_fn:
        bc_fn(oc)
    oc.set_fields(*tiled_fields(smooth_fields, long.array("C").reshape(-1, 3), 1.0))
    oc.step(steps)
    idx = np.arange(long.nCells).reshape(nz, ny, 3 * nx)[:, :, nx: 2 * nx].reshape(-1)
    for f in ("rho", "U", "p", "e"):
        a, b = per.field(f, g.nCells), oc.field(f)[idx]
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (stencil, f, np.abs(a - b).max())


def conserved(case, V, n):
    rho, U, rhoE = case.field("rho")[:n], case.field("U")[:n], case.field("rhoE")[:n]
    return np.array([(rho * V).sum(), *((rho[:, None] * U) * V[:, None]).sum(axis=0), (rhoE * V).sum()])


def test_triply_periodic_box_conserves_mass_momentum_and_energy():
    g = periodic_box((6, 5, 4), (True, True, True))
    ext = g.unroll_cyclic()
    assert ext.halo_slots == 26                                   # 6 sides, 12 edges, 8 corners
    per = OraclePeriodic(ext, q.default_options(stencil="GaussVolPoint", deltaT=2e-3, mu=1e-3))
    C = g.array("C").reshape(-1, 3)
    U, T, p = smooth_fields(C)
    U[:, 2] += 0.04 * np.sin(2 * np.pi * C[:, 1])
    T = T + 0.03 * np.sin(2 * np.pi * C[:, 2])
    per.set_fields(U, T, p)
    V = g.array("V")
    before = conserved(per.case, V, g.nCells)
    per.step(12)
    after = conserved(per.case, V, g.nCells)
    scale = np.array([before[0], before[0], before[0], before[0], before[4]])
    assert (np.abs(after - before) <= 1e-13 * scale).all(), (after - before) / scale
    assert np.abs(per.case.field("rho")[:g.nCells] - 1.0).max() > 1e-3      # (something happened)


def test_a_pulse_leaves_through_one_half_and_re_enters_through_the_other():
    nx = 40
    g = periodic_box((nx, 3, 3), (True, True, True), hi=(1.0, 0.075, 0.075))
    ext = g.unroll_cyclic()
    C = g.array("C").reshape(-1, 3)
    U = np.zeros_like(C); U[:, 0] = 2.5                            # supersonic carrier (c = 1): everything moves to the right
    T = np.ones(g.nCells)
    p = 1.0 + 0.05 * np.exp(-((C[:, 0] - 0.85) / 0.05) ** 2)
    per = OraclePeriodic(ext, q.default_options(stencil="GaussVolPoint", deltaT=1e-3))
    per.set_fields(U, T, p)
    x0 = C[np.argmax(per.field("p", g.nCells)), 0]
    per.step(200)     # t = 0.2: the pressure pulse has split into its two acoustic halves, at u + c = 3.5 -> 0.85 + 0.70 = 1.55 -> 0.55 and at
    pn = per.field("p", g.nCells)                                  # u - c = 1.5 -> 0.85 + 0.30 = 1.15 -> 0.15: both have left through xMax and re-entered at xMin
    x1 = C[np.argmax(pn), 0]
    assert x0 > 0.8 and 0.05 < x1 < 0.65, (x0, x1)
    assert pn.max() - 1.0 > 5e-3                                   # still a pulse, not noise
    # the same pulse in a box whose ends are ordinary (zeroGradient) patches just leaves: nothing like it is found in x < 0.65 then
    pt = [G, G, CYC, CYC, CYC, CYC]
    h = q.PolyMesh.box(nx, 3, 3, hi=(1.0, 0.075, 0.075), patch_types=pt)
    he = h.unroll_cyclic()
    out = OraclePeriodic(he, q.default_options(stencil="GaussVolPoint", deltaT=1e-3))
    out.set_fields(U, T, p)
    out.step(200)
    po = out.field("p", h.nCells)
    assert po[C[:, 0] < 0.65].max() - 1.0 < 0.2 * (pn.max() - 1.0), (po.max(), pn.max())


# ---- off the uniform box -------------------------------------------------------------------------------------------------------------
JITTER = 0.15


def cell_points(prim, n_cells):
    """the point labels of every cell, from the faces"""
    fo, fp, own, nei = prim["faceOffsets"], prim["facePoints"], prim["owner"], prim["neighbour"]
    pts = [set() for _ in range(n_cells)]
    for f in range(own.size):
        face = fp[fo[f]: fo[f + 1]]
        pts[own[f]].update(face)
        if f < nei.size:
            pts[nei[f]].update(face)
    return pts


def test_periodic_box_applies_its_jitter():
    a, b = periodic_box((6, 5, 4), (True, True, True)), periodic_box((6, 5, 4), (True, True, True), jitter=JITTER)
    moved = np.abs(a.array("points") - b.array("points")).reshape(-1, 3).max(axis=1)
    assert (moved > 0).sum() == 5 * 4 * 3 and moved.max() > 0.05 * JITTER / 6       # every interior point, and no other
    assert np.ptp(b.array("V")) > 0.05 * b.array("V").mean()


@pytest.mark.parametrize("periodic,slots", [((True, False, False), 2), ((True, True, False), 8), ((True, True, True), 26)])
def test_unrolled_jittered_box_has_translated_copies(periodic, slots):
    """no two cells of the jittered box are translates of each other, so a copy that took the wrong original, or the right one's geometry
    with the wrong shift, shows: per slot, centres, points and volumes of the copies are their originals' moved by ONE lattice vector"""
    g = periodic_box((6, 5, 4), periodic, jitter=JITTER)
    ext = g.unroll_cyclic()
    n = g.nCells
    assert ext.halo_slots == slots and np.array_equal(ext.array("points")[:3 * g.nPoints], g.array("points"))
    self_slot = ext.array("haloSelf")
    cg, C, V, X = ext.array("cellGlobal"), ext.array("C").reshape(-1, 3), ext.array("V"), ext.array("points").reshape(-1, 3)
    assert np.abs(V[:n] - g.array("V")).max() <= 1e-13 * V.max() and np.abs(C[:n] - g.array("C").reshape(-1, 3)).max() < 1e-13   # (the real cells' own)
    pts = cell_points(ext.primitives(), ext.nCells)
    seen = np.zeros(ext.nCells, dtype=bool)
    for k in range(slots):
        ghost, send = ext.array(f"haloGhost{k}"), ext.array(f"haloSend{int(self_slot[k])}")
        assert (ghost >= n).all() and (send < n).all() and np.array_equal(cg[ghost], send)
        seen[ghost] = True
        shift = C[ghost] - C[send]
        lattice = np.round(shift[0])
        assert np.abs(shift - lattice).max() < 1e-12 and np.abs(lattice).max() == 1.0
        assert all(lattice[d] == 0 for d in range(3) if not periodic[d])
        assert np.abs(V[ghost] - V[send]).max() <= 1e-13 * V.max()
        for gcell, orig in zip(ghost, send):
            a = X[sorted(pts[gcell])]
            b = X[sorted(pts[orig])] + lattice
            assert a.shape == b.shape == (8, 3)
            a, b = a[np.lexsort(np.round(a, 9).T)], b[np.lexsort(np.round(b, 9).T)]
            assert np.abs(a - b).max() < 1e-12, (k, gcell, orig)
    assert seen[n:].all() and not seen[:n].any()          # every copy belongs to a slot


def test_triply_periodic_jittered_box_conserves_mass_momentum_and_energy():
    """test_triply_periodic_box_conserves_mass_momentum_and_energy off the uniform box: same steps, same 1e-13"""
    g = periodic_box((6, 5, 4), (True, True, True), jitter=JITTER)
    ext = g.unroll_cyclic()
    assert ext.halo_slots == 26
    per = OraclePeriodic(ext, q.default_options(stencil="GaussVolPoint", deltaT=2e-3, mu=1e-3))
    C = g.array("C").reshape(-1, 3)
    U, T, p = smooth_fields(C)
    U[:, 2] += 0.04 * np.sin(2 * np.pi * C[:, 1])
    T = T + 0.03 * np.sin(2 * np.pi * C[:, 2])
    per.set_fields(U, T, p)
    V = g.array("V")
    before = conserved(per.case, V, g.nCells)
    per.step(12)
    after = conserved(per.case, V, g.nCells)
    scale = np.array([before[0], before[0], before[0], before[0], before[4]])
    print("conservation defect / scale:", (after - before) / scale)
    assert (np.abs(after - before) <= 1e-13 * scale).all(), (after - before) / scale
    assert np.abs(per.case.field("rho")[:g.nCells] - 1.0).max() > 1e-3


def three_boxes_in_a_row(g, nx, ny, nz):
    """the box of 3 nx x ny x nz cells on [-1, 2) x [0, 1)^2 whose points are three copies of g's, translated by -1, 0, +1 in x, the
    coincident points of the seams merged (g's boundary points were not jittered: they coincide exactly); built from arrays, not by
    qgd_mesh_unroll_cyclic"""
    long = q.PolyMesh.box(3 * nx, ny, nz, lo=(-1.0, 0.0, 0.0), hi=(2.0, 1.0, 1.0))
    prim = long.primitives()
    Xl = prim["points"].reshape(nz + 1, ny + 1, 3 * nx + 1, 3)
    Xg = g.array("points").reshape(nz + 1, ny + 1, nx + 1, 3)
    i = np.arange(3 * nx + 1)
    tile, src = np.minimum(i // nx, 2), i - nx * np.minimum(i // nx, 2)
    new = Xg[:, :, src, :].copy()
    new[..., 0] += (tile - 1.0)[None, None, :]
    flat = q.PolyMesh.box(nx, ny, nz, patch_types=[CYC, CYC, G, G, G, G]).array("points").reshape(Xg.shape)[:, :, src, :].copy()
    flat[..., 0] += (tile - 1.0)[None, None, :]
    assert np.abs(flat - Xl).max() < 1e-14                 # (the point numbering is the one assumed: the unjittered tiles ARE the long box)
    assert np.abs(new - Xl).max() > 1e-3
    return q.PolyMesh.from_arrays(new.reshape(-1), prim["faceOffsets"], prim["facePoints"], prim["owner"], prim["neighbour"], prim["nCells"],
                                  prim["patchStart"], prim["patchSize"], prim["patchType"])


@pytest.mark.parametrize("stencil,bc_fn", [("GaussVolPoint", None), ("GaussVolPoint", wall_bcs), ("reduced", None)])
def test_jittered_periodic_box_is_the_middle_of_three_of_its_kind(stencil, bc_fn):
    """test_periodic_box_is_the_middle_of_a_three_times_longer_box off the uniform box; the one check of the unrolled geometry that does not
    go through qgd_mesh_unroll_cyclic.  Same 1e-12."""
    nx, ny, nz, steps = 8, 5, 4, 3
    opt = q.default_options(stencil=stencil, deltaT=2e-3, mu=1e-3)
    g = periodic_box((nx, ny, nz), (True, False, False), jitter=JITTER)
    ext = g.unroll_cyclic()
    per = OraclePeriodic(ext, opt, bc_fn)
    per.set_fields(*smooth_fields(g.array("C").reshape(-1, 3)))
    per.step(steps)
    long = three_boxes_in_a_row(g, nx, ny, nz)
    idx = np.arange(long.nCells).reshape(nz, ny, 3 * nx)[:, :, nx: 2 * nx].reshape(-1)
    Cl = long.array("C").reshape(-1, 3)
    assert np.abs(Cl[idx] - g.array("C").reshape(-1, 3)).max() < 1e-13 and np.abs(long.array("V")[idx] - g.array("V")).max() < 1e-15
    oc = OracleCase(OracleMesh(long.primitives()), opt)
    if bc_fn:
        bc_fn(oc)
    oc.set_fields(*tiled_fields(smooth_fields, Cl, 1.0))
    oc.step(steps)
    for f in ("rho", "U", "p", "e"):
        a, b = per.field(f, g.nCells), oc.field(f)[idx]
        print(stencil, f, np.abs(a - b).max() / np.abs(b).max())
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (stencil, f, np.abs(a - b).max())


def test_application_refuses_a_periodic_case_with_a_nonuniform_coefficient_file_by_name(tmp_path):
    """QGDFoam.run on a cyclic case with a non-uniform alphaQGD file: refused like foamfile.load_case refuses it, before a device exists"""
    import os
    from qgdsolver_amd import QGDFoam, foamfile as ff

    case_dir = str(tmp_path)
    mesh, _ = write_periodic_case(case_dir)
    a = 0.4 + 0.1 * np.sin(2 * np.pi * mesh.array("C").reshape(-1, 3)[:, 0])
    cyc = ("cyclic", None)
    patches = {"left": cyc, "right": cyc, **{k: ("zeroGradient", None) for k in ("bottom", "top", "back", "front")}}
    for name in ("alphaQGD", "ScQGD"):
        path = os.path.join(case_dir, "0", name)
        ff.write_field(path, mesh, name, a, patches)
        with pytest.raises(ff.FoamFileError, match="uniform alphaQGD / ScQGD"):
            QGDFoam.run(case_dir, n_steps=1, log=lambda *a, **k: None)
        with pytest.raises(ff.FoamFileError, match="uniform alphaQGD / ScQGD"):
            ff.load_case(case_dir)
        os.remove(path)



# ---- the device ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["fused", "kernels"])
@pytest.mark.parametrize("periodic,bc_fn,stencil", [((True, False, False), wall_bcs, "GaussVolPoint"), ((True, True, True), None, "GaussVolPoint"),
                                                    ((True, True, False), None, "reduced")])
def test_device_steps_a_periodic_case_like_the_oracle(periodic, bc_fn, stencil, arm):
    if arm == "fused" and stencil != "GaussVolPoint":
        pytest.skip("the fused step serves GaussVolPoint")
    device_against_oracle(periodic, bc_fn, stencil, arm, 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("periodic,bc_fn,stencil,arm", [((True, False, False), wall_bcs, "GaussVolPoint", "fused"), ((True, False, False), wall_bcs, "GaussVolPoint", "kernels"),
                                                        ((True, True, True), None, "GaussVolPoint", "fused"), ((True, True, True), None, "GaussVolPoint", "kernels"),
                                                        ((True, True, False), None, "reduced", "kernels")])
def test_device_steps_a_jittered_periodic_case_like_the_oracle(periodic, bc_fn, stencil, arm):
    """the same on a box whose interior points are jittered: nothing in a copy's centre, volume or vertex weights cancels by symmetry"""
    device_against_oracle(periodic, bc_fn, stencil, arm, JITTER)


def device_against_oracle(periodic, bc_fn, stencil, arm, jitter):
    g = periodic_box((10, 8, 6), periodic, jitter=jitter)
    ext = g.unroll_cyclic()
    opt = q.default_options(stencil=stencil, deltaT=1e-3, mu=1e-3)
    U, T, p = smooth_fields(g.array("C").reshape(-1, 3))
    per = OraclePeriodic(ext, opt, bc_fn)
    per.set_fields(U, T, p)
    dev = q.Device(ext, fused_tables="any" if arm == "fused" else False)
    gc = q.QGDFoamCase(dev, opt)
    assert gc.fused_info()["fused"] == (arm == "fused")
    if bc_fn:
        bc_fn(gc)
    cg = ext.array("cellGlobal")
    gc.set_fields(U[cg], T[cg], p[cg])
    for chunk in (1, 9):
        gc.step(chunk)                                             # plain step: the library refreshes the copies itself
        per.step(chunk)
        for f in ("rho", "U", "p", "e"):
            a, b = gc.field(f)[:g.nCells], per.field(f, g.nCells)
            assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (periodic, stencil, arm, jitter, f, np.abs(a - b).max() / np.abs(b).max())
        # the copies hold their originals' records
        assert np.array_equal(gc.field("rho")[g.nCells:], gc.field("rho")[cg[g.nCells:]])
    with pytest.raises(q.QgdError, match="implicitDiffusion"):
        ic = q.QGDFoamCase(dev, q.default_options(stencil=stencil, deltaT=1e-3, mu=1e-3, implicitDiffusion=1))
        ic.set_fields(U[cg], T[cg], p[cg])
        ic.step(1)
    from qgdsolver_amd import qhdfoam
    with pytest.raises(q.QgdError, match="unrolled"):
        qhdfoam.QHDFoamCase(dev, qhdfoam.qhd_options(stencil=stencil, deltaT=1e-3))
    gc.close(); dev.close()


# ---- the copies belong to the library ---------------------------------------------------------------------------------------------------
FLUX_TOL = 1e-11      # tests/test_case_parity_gpu.py
FACE_FIELDS = ["phiJm", "phiJmU", "phiP", "phiPi", "phiJmH", "phiQ", "phiPiU", "phiwStar", "phi", "tauQGDf", "hQGDf", "gradUf", "gradef", "gradRhof", "gradPf"]


def periodic_pair(periodic, bc_fn, arm, jitter=0.0, **opt):
    g = periodic_box((10, 8, 6), periodic, jitter=jitter)
    ext = g.unroll_cyclic()
    options = q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3, **opt)
    per = OraclePeriodic(ext, options, bc_fn)
    dev = q.Device(ext, fused_tables="any" if arm == "fused" else False)
    gc = q.QGDFoamCase(dev, options)
    assert gc.fused_info()["fused"] == (arm == "fused")
    if bc_fn:
        bc_fn(gc)
    return g, ext, per, dev, gc


def with_wrong_copies(ext, n, U, T, p, how):
    """real-cell values for the real cells; the copies get values no computation may see"""
    cg = ext.array("cellGlobal")
    Ue, Te, pe = U[cg].copy(), T[cg].copy(), p[cg].copy()
    if how == "nan":
        Ue[n:], Te[n:], pe[n:] = np.nan, np.nan, np.nan
    else:
        Ue[n:], Te[n:], pe[n:] = 0.0, 2.0, 0.5
    return Ue, Te, pe


def faces_of_real_cells(ext, n):
    """every face with a real cell on either side: the real mesh's internal faces, the glued seam faces, the real patch faces"""
    own, nei = ext.array("owner"), ext.array("neighbour")
    real = own < n
    real[:nei.size] |= nei < n
    return real


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["nan", "other values"])
@pytest.mark.parametrize("periodic,bc_fn", [((True, False, False), wall_bcs), ((True, True, True), None)])
def test_update_fluxes_does_not_read_what_the_caller_put_into_the_copies(periodic, bc_fn, how):
    """qgd_case_set_fields with wrong values in the copies, then qgd_case_update_fluxes: the face fields of every face of the real cells, the
    glued seam faces included, are the oracle's (copies refreshed by hand) at FLUX_TOL.
    (Before qgd_case_update_fluxes refreshed the copies itself, this failed on the first field, phiJm: not finite with NaN in the copies, and
    off by the size of the field itself with other values.)"""
    g, ext, per, dev, gc = periodic_pair(periodic, bc_fn, "kernels", jitter=JITTER)
    n = g.nCells
    U, T, p = smooth_fields(g.array("C").reshape(-1, 3))
    per.set_fields(U, T, p)
    gc.set_fields(*with_wrong_copies(ext, n, U, T, p, how))
    gc.updateFluxes()
    per.update_fluxes()
    real = faces_of_real_cells(ext, n)
    assert real.sum() > g.nFaces - 1 - sum(g.array("patchSize")[i] for i in range(g.nPatches) if g.array("patchType")[i] == CYC) // 2 - 1
    for f in FACE_FIELDS:
        a, b = gc.field(f), per.case.field(f)
        a, b = a.reshape(ext.nFaces, -1)[real], b.reshape(ext.nFaces, -1)[real]
        assert np.isfinite(a).all(), (periodic, how, f)
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
        print(f"{periodic} {how} {f}: {err:.3e}")
        assert err <= FLUX_TOL, (periodic, how, f, err)
    # ... and a step from there is the oracle's too
    gc.step(2); per.step(2)
    for f in ("rho", "U", "p", "e"):
        a, b = gc.field(f)[:n], per.field(f, n)
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (periodic, how, f)
    gc.close(); dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["fused", "kernels"])
def test_stepping_a_periodic_device_by_phases_is_refused_by_name(arm):
    """qgd_case_step_phase knows nothing of the copies (nothing would refresh them between two phases): on a periodic device it is refused,
    by name, and leaves the case as it was -- five plain steps afterwards are OraclePeriodic.step(5) (include/qgd_amd.h qgd_mesh_unroll_cyclic)"""
    g, ext, per, dev, gc = periodic_pair((True, True, False), None, arm)
    n = g.nCells
    U, T, p = smooth_fields(g.array("C").reshape(-1, 3))
    per.set_fields(U, T, p)
    cg = ext.array("cellGlobal")
    gc.set_fields(U[cg], T[cg], p[cg])
    for phase in (0, 1, 3, 10):
        with pytest.raises(q.QgdError, match="periodic device"):
            gc.step_phase(phase)
    gc.step(5); per.step(5)
    for f in ("rho", "U", "p", "e"):
        a, b = gc.field(f)[:n], per.field(f, n)
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (arm, f)
    gc.close(); dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["fused", "kernels"])
def test_set_bc_after_stepping_a_periodic_device(arm):
    """step(3), then another condition on a wall patch: the case asks for set_fields again (as on every mesh), and after it -- handed the
    current state for the real cells and zeros for the copies -- updateFluxes and a step are the oracle's doing the same"""
    g, ext, per, dev, gc = periodic_pair((True, False, False), wall_bcs, arm, jitter=JITTER)
    n = g.nCells
    U, T, p = smooth_fields(g.array("C").reshape(-1, 3))
    per.set_fields(U, T, p)
    cg = ext.array("cellGlobal")
    gc.set_fields(U[cg], T[cg], p[cg])
    gc.step(3); per.step(3)

    def new_wall(case):
        case.set_bc(3, U=("fixedValue", (0.1, 0.0, 0.0)), T=("fixedValue", 1.05), p=("zeroGradient", None))
    new_wall(gc); new_wall(per.case)
    with pytest.raises(q.QgdError, match="set_fields"):
        gc.updateFluxes()
    with pytest.raises(q.QgdError, match="set_fields"):
        gc.step(1)
    U3, T3, p3 = per.field("U", n).copy(), per.field("T", n).copy(), per.field("p", n).copy()
    for f, want in (("U", U3), ("T", T3), ("p", p3)):
        assert np.abs(gc.field(f)[:n] - want).max() <= 1e-10 * np.abs(want).max(), f
    per.set_fields(U3, T3, p3)
    gc.set_fields(*with_wrong_copies(ext, n, U3, T3, p3, "other values"))
    gc.updateFluxes(); per.update_fluxes()
    real = faces_of_real_cells(ext, n)
    for f in FACE_FIELDS:
        a, b = gc.field(f).reshape(ext.nFaces, -1)[real], per.case.field(f).reshape(ext.nFaces, -1)[real]
        assert np.abs(a - b).max() <= FLUX_TOL * max(np.abs(b).max(), 1e-300), (arm, f)
    gc.step(1); per.step(1)
    for f in ("rho", "U", "p", "e"):
        a, b = gc.field(f)[:n], per.field(f, n)
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (arm, f)
    gc.close(); dev.close()


def write_periodic_case(case_dir, n=(10, 6, 4)):
    """a channel periodic in x between slip walls (qgdFlux pressure) in y, zeroGradient in z, written the way a QGDFoam user would: the
    dictionaries of the forwardStep test case, this mesh (`neighbourPatch` entries in constant/polyMesh/boundary) and non-uniform fields"""
    import os
    import shutil
    from qgdsolver_amd import foamfile as ff
    from test_foamfile import write_step_case

    write_step_case(case_dir, "GaussVolPoint")
    shutil.rmtree(os.path.join(case_dir, "constant", "polyMesh"))
    mesh = periodic_box(n, (True, False, False))
    mesh.patch_names = ["left", "right", "bottom", "top", "back", "front"]
    mesh.cyclic_pairs = [(0, 1)]
    ff.write_polymesh(mesh, os.path.join(case_dir, "constant", "polyMesh"))
    U, T, p = smooth_fields(mesh.array("C").reshape(-1, 3))
    cyc = ("cyclic", None)
    ff.write_field(os.path.join(case_dir, "0", "U"), mesh, "U", U,
                   {"left": cyc, "right": cyc, "bottom": ("slip", None), "top": ("slip", None), "back": ("zeroGradient", None), "front": ("zeroGradient", None)})
    ff.write_field(os.path.join(case_dir, "0", "T"), mesh, "T", T,
                   {"left": cyc, "right": cyc, **{k: ("zeroGradient", None) for k in ("bottom", "top", "back", "front")}})
    ff.write_field(os.path.join(case_dir, "0", "p"), mesh, "p", p,
                   {"left": cyc, "right": cyc, "bottom": ("qgdFlux", None), "top": ("qgdFlux", None), "back": ("zeroGradient", None), "front": ("zeroGradient", None)})
    return mesh, (U, T, p)


def test_reader_pairs_the_halves_and_refuses_what_is_not_served(tmp_path):
    from qgdsolver_amd import foamfile as ff

    mesh, _ = write_periodic_case(str(tmp_path / "ok"))
    m2, opt, fields, bcs = ff.read_case_setup(str(tmp_path / "ok"))
    assert m2.cyclic_pairs == [(0, 1)] and bcs[0]["U"] == ("none", None) and bcs[2]["p"] == ("qgdFlux", None)
    ext = m2.unroll_cyclic(m2.cyclic_pairs)
    assert ext.nCells == mesh.nCells + 2 * 6 * 4 and np.array_equal(ext.array("haloSelf"), [1, 0])
    # a half that does not name its partner, a rotational pair, a field that is not `cyclic` on a cyclic patch
    bpath = str(tmp_path / "ok" / "constant" / "polyMesh" / "boundary")
    text = open(bpath).read()
    assert "neighbourPatch  right;" in text
    for bad, match in ((text.replace("neighbourPatch  right;", ""), "neighbourPatch"),
                       (text.replace("neighbourPatch  right;", "neighbourPatch right; transform rotational;"), "rotational")):
        open(bpath, "w").write(bad)
        with pytest.raises(ff.FoamFileError, match=match):
            ff.read_case_setup(str(tmp_path / "ok"))
    open(bpath, "w").write(text)
    upath = str(tmp_path / "ok" / "0" / "U")
    utext = open(upath).read()
    open(upath, "w").write(utext.replace("cyclic", "zeroGradient", 1))
    with pytest.raises(ff.FoamFileError, match="inconsistent patch and patchField types"):
        ff.read_case_setup(str(tmp_path / "ok"))


@pytest.mark.gpu
def test_application_runs_a_periodic_case_directory(tmp_path):
    """python -m qgdsolver_amd.QGDFoam on a case with a cyclic pair: the written fields are the oracle's (copies refreshed by hand), cell for cell"""
    import os
    from qgdsolver_amd import QGDFoam, foamfile as ff

    case_dir = str(tmp_path)
    mesh, (U, T, p) = write_periodic_case(case_dir)
    cd = os.path.join(case_dir, "system", "controlDict")
    text = open(cd).read()
    open(cd, "w").write(text.replace("endTime 1;", "endTime 0.01;") + "writeControl timeStep;\nwriteInterval 10;\n")
    dev, case, written = QGDFoam.run(case_dir, n_steps=20, log=lambda *a, **k: None)
    assert written == ["0.005", "0.01"]
    opt = q.default_options(stencil="GaussVolPoint", deltaT=5e-4, R=1 / 1.4, Cv=1 / 1.4 / 0.4, mu=0.0, Pr=1.0, ScQGD=1.0, PrQGD=1.0, alphaQGD=0.5)
    per = OraclePeriodic(mesh.unroll_cyclic([(0, 1)]), opt, wall_bcs)
    per.set_fields(U, T, p)
    per.step(20)
    for name in ("U", "T", "p", "rho"):
        vals, patches = ff.read_field(os.path.join(case_dir, "0.01", name), mesh)
        want = per.field(name, mesh.nCells)
        assert np.abs(vals.reshape(want.shape) - want).max() <= 1e-10 * np.abs(want).max(), name
        assert patches["left"]["type"] == "cyclic"
    case.close(); dev.close()
