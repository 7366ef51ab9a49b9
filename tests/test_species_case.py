"""CPU: properties of the host replay of a QGDFoam case with species (tests/species_ref.py), the reference the device step is held to
in tests/test_species_case_gpu.py.  Compositions stay in [0.1, 0.6], so nothing below hides behind Yi.max(0)."""
import numpy as np
import pytest

import qgdsolver_amd as q

import cases
from oracle import OracleCase
from species_ref import SpeciesReplay
from util import make_mesh, oracle_mesh_of

CASES = [("box654_poly", "GaussVolPoint", dict(deltaT=1e-3, mu=1e-3)), ("plane2d_jitter", "leastSquares", dict(deltaT=5e-4, mu=1e-3))]
INERT = 2


def flow_bcs(mesh, case):
    """zero-gradient walls; the patches of an empty direction carry nothing"""
    for patch, t in enumerate(mesh.array("patchType")):
        if t != 0:
            case.set_bc(patch, U=("none", None), T=("none", None), p=("none", None))


def flow_fields(C, moving=True):
    U, T, p = cases.box_initial_fields(C)
    r2 = (C[:, 0] - 0.5) ** 2 + (C[:, 1] - 0.4) ** 2
    p = 1.0 + 0.1 * np.exp(-r2 / 0.02)
    U = np.array(U, dtype=float)
    U[:, 0] += 0.3
    U[:, 1] -= 0.1
    if not moving:
        return np.zeros_like(U), np.ones_like(T), np.ones_like(p)
    return U, T, p


def smooth_composition(C):
    """four species, every value (the inert one's included) in [0.1, 0.6]; species 1 is uniform"""
    y0 = 0.2 + 0.1 * np.sin(2 * np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1])
    y1 = np.full(C.shape[0], 0.2)
    y3 = 0.2 + 0.1 * np.cos(3.0 * C[:, 0] + 2.0 * C[:, 1])
    Y = [y0, y1, 1.0 - y0 - y1 - y3, y3]
    assert all(y.min() >= 0.1 and y.max() <= 0.6 for y in Y)
    return Y


def oracle_pair(kind, scheme, opt, moving=True):
    mesh = make_mesh(kind)
    om = oracle_mesh_of(mesh)
    oc = OracleCase(om, q.default_options(stencil=scheme, **opt))
    flow_bcs(mesh, oc)
    C = mesh.array("C").reshape(-1, 3)
    oc.set_fields(*flow_fields(C, moving))
    return mesh, om, oc, C


@pytest.mark.parametrize("kind,scheme,opt", CASES)
@pytest.mark.parametrize("adjust", [0, 1])
def test_update_fluxes_between_steps_leaves_the_trajectory_alone(kind, scheme, opt, adjust):
    """the replay calls updateFluxes() before every step to read the face fields: the oracle's states must be, bit for bit, those of step(n)"""
    o = dict(opt, adjustTimeStep=adjust, maxCo=0.3)
    _, _, a, _ = oracle_pair(kind, scheme, o)
    _, _, b, _ = oracle_pair(kind, scheme, o)
    a.step(3)
    for _ in range(3):
        b.updateFluxes()
        b.step(1)
    for name in ("rho", "U", "p", "e", "rhoE", "rho.boundary", "U.boundary", "p.boundary"):
        assert np.array_equal(a.field(name), b.field(name)), (kind, name)
    assert a.info() == b.info()


def test_with_qgdflux_walls_the_replay_reads_its_face_fields_from_a_second_case():
    """updateFluxes() re-evaluates p's qgdFlux boundary condition: between steps it moves the oracle's trajectory (far above rounding), so on
    such a case the replay leaves the main case alone and reads the face fields from a second one brought to the same state"""
    def new():
        mesh = make_mesh("step2d")
        oc = OracleCase(oracle_mesh_of(mesh), q.default_options(stencil="GaussVolPoint", deltaT=5e-4, mu=1e-3))
        cases.forward_step_bcs(oc)
        C = mesh.array("C").reshape(-1, 3)
        U = np.zeros((mesh.nCells, 3))
        U[:, 0] = 3.0
        oc.set_fields(U, 1.0 + 0.05 * np.sin(2.0 * C[:, 0]) * np.cos(3.0 * C[:, 1]), 1.0 + 0.05 * np.cos(1.5 * C[:, 0] + C[:, 1]))
        return mesh, oc
    _, a = new()
    _, b = new()
    mesh, c = new()
    a.step(3)
    for _ in range(3):
        b.updateFluxes()
        b.step(1)
    assert np.abs(a.field("p") - b.field("p")).max() > 1e-9
    C = mesh.array("C").reshape(-1, 3)
    rep = SpeciesReplay(mesh, oracle_mesh_of(mesh), c, "GaussVolPoint", smooth_composition(C), INERT, fresh=lambda: new()[1])
    Y = rep.step(3)
    for name in ("rho", "U", "p", "e", "rhoE"):
        assert np.array_equal(a.field(name), c.field(name)), name
    assert rep.steps == 3 and min(float(y.min()) for y in Y) > 0.0 and np.abs(sum(Y) - 1.0).max() <= 1e-14


@pytest.mark.parametrize("kind,scheme,opt", CASES)
def test_species_mass_budget_uniformity_and_no_clip(kind, scheme, opt):
    mesh, om, oc, C = oracle_pair(kind, scheme, opt)
    V = mesh.array("V")
    nif = mesh.nInternalFaces
    rep = SpeciesReplay(mesh, om, oc, scheme, smooth_composition(C), INERT, ScNumbers=[0.7, 1.0, 1.0, 1.3])
    for _ in range(3):
        rho0 = oc.field("rho")
        m0 = [float(np.sum(rho0 * y * V)) for y in rep.Y]
        Y = rep.step(1)
        rho1 = oc.field("rho")
        for i in (0, 1, 3):
            # zero-gradient walls let the flow through: what crosses them is phiJmY_i (the laplacian flux of a zero-gradient patch is zero), so
            # the mass of a transported species changes by exactly -deltaT times that; everything inside telescopes
            through = float(np.sum(rep.phiJmY[i][nif:]))
            m1 = float(np.sum(rho1 * Y[i] * V))
            assert abs(m1 - m0[i] + rep.deltaT * through) <= 1e-13 * m0[i], (kind, i, m1 - m0[i], rep.deltaT * through)
        assert np.abs(Y[1] - 0.2).max() <= 1e-13 * 0.2, (kind, np.abs(Y[1] - 0.2).max())      # a uniform species stays uniform
        assert min(float(y.min()) for y in Y) > 0.0                                            # nothing was clipped, the inert one included
        assert np.abs(sum(Y) - 1.0).max() <= 1e-14


@pytest.mark.parametrize("kind,scheme,opt", CASES)
def test_species_mass_is_conserved_in_a_closed_box(kind, scheme, opt):
    """gas at rest at uniform pressure and temperature: no mass flux through any face, the walls included (phiJm is zero up to the rounding of
    the vertex weights, 1e-17, five orders below the bar), and the species diffuse (mu > 0) between zero-gradient walls: sum rho Y_i V of
    every transported species is conserved"""
    mesh, om, oc, C = oracle_pair(kind, scheme, opt, moving=False)
    V = mesh.array("V")
    Y0 = smooth_composition(C)
    rep = SpeciesReplay(mesh, om, oc, scheme, Y0, INERT, ScNumbers=[0.7, 1.0, 1.0, 1.3])
    rho0 = oc.field("rho")
    Y = rep.step(3)
    assert np.abs(oc.field("phiJm")).max() <= 1e-15
    rho1 = oc.field("rho")
    for i in (0, 1, 3):
        m0, m1 = float(np.sum(rho0 * Y0[i] * V)), float(np.sum(rho1 * Y[i] * V))
        assert abs(m1 - m0) <= 1e-13 * m0, (kind, i, m1 - m0)
    assert np.abs(Y[0] - Y0[0]).max() > 1e-9     # (the laplacian did move something)
    assert min(float(y.min()) for y in Y) > 0.0
