"""scalarTransportQHDFoam resident on the device (qgdsolver_amd.scalarfoam, qgd_scalar_case_*) against the numpy restatement of the
listing's step (tests/scalar_ref.py), the case-directory reader / writer and the application.

Bounds: 1e-10 of the field's maximum for T after an iterative solve and 1e-11 for face fields are the ones this project holds its
iterative branches and face fields to (tests/test_implicit_diffusion.py, FLUX_TOL); the analytic bounds of config 1 are those of
tests/test_config1_scalar_transport.py.
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L, foamfile as ff

import test_config1_scalar_transport as c1
from scalar_ref import ScalarRef, delta_t_rule
from util import make_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "FoamFile {{ version 2.0; format ascii; class {cls}; object {obj}; }}\n"
T_TOL, FLUX_TOL = 1e-10, 1e-11
TAU, RHO0, PR = 2e-3, 1.2, 0.7


def smooth_fields(mesh):
    """a smooth velocity that is NOT divergence-free and a smooth T; components along empty directions are zero"""
    C = mesh.array("C").reshape(-1, 3)
    x, y, z = C[:, 0], C[:, 1], C[:, 2]
    pt = mesh.array("patchType")
    live = [int(pt[2 * d]) != L.PATCH_EMPTY for d in range(3)]
    U = np.stack([1.0 + 0.3 * np.sin(2.0 * x + y), 0.2 * np.cos(3.0 * y + x) * live[1], (0.1 + 0.15 * x * z) * live[2]], axis=1)
    T = 1.0 + 0.5 * np.sin(3.0 * x) * np.cos(2.0 * y * live[1]) + 0.2 * z * live[2]
    return U, T


def mixed_bcs(mesh):
    """fixedValue inlet (patch 0), zeroGradient outlet (patch 1), one slip wall for U (patch 2 where it is no empty patch), zeroGradient elsewhere"""
    pt = mesh.array("patchType")
    bcs = []
    for i in range(mesh.nPatches):
        if i == 0:
            bcs.append({"U": ("fixedValue", (1.1, 0.05, 0.0)), "T": ("fixedValue", 1.3)})
        elif i == 2 and int(pt[i]) == L.PATCH_GENERIC:
            bcs.append({"U": ("slip", None), "T": ("zeroGradient", None)})
        else:
            bcs.append({"U": ("zeroGradient", None), "T": ("zeroGradient", None)})
    return bcs


def device_case(mesh, stencil, bcs, U, T, **opt):
    from qgdsolver_amd import scalarfoam
    dev = q.Device(mesh, fused_tables=False)
    o = dict(stencil=stencil, tauModel="constTau", Tau=TAU, rho0=RHO0, Pr=PR, mu=1e-2, deltaT=1e-3, implicitTol=1e-13, implicitMaxIter=2000)
    o.update(opt)
    case = scalarfoam.ScalarTransportQHDCase(dev, scalarfoam.scalar_options(**o))
    for i, bc in enumerate(bcs):
        case.set_bc(i, U=bc["U"], T=bc["T"])
    case.set_fields(U, T)
    return dev, case


def close(a, b, tol):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= tol * max(np.abs(b).max(), 1e-300)


# ---- CPU: the restatement itself ----------------------------------------------------------------------------------------------------------
def config1_ref():
    G, E = L.PATCH_GENERIC, L.PATCH_EMPTY
    mesh = q.PolyMesh.box(c1.N, 1, 1, hi=(c1.LX, 0.01, 0.01), patch_types=[G, G, E, E, E, E])
    x = mesh.array("C").reshape(-1, 3)[:, 0]
    T0 = np.exp(-((x - 0.3) / 0.05) ** 2)
    U = np.tile([c1.UX, 0.0, 0.0], (c1.N, 1))
    bcs = [{"U": ("fixedValue", (c1.UX, 0.0, 0.0)), "T": ("fixedValue", 0.0)}, {"U": ("fixedValue", (c1.UX, 0.0, 0.0)), "T": ("zeroGradient", None)}]
    bcs += [{"U": ("zeroGradient", None), "T": ("zeroGradient", None)}] * 4
    return mesh, x, U, T0, bcs


_config1_cache = {}


def config1_restated():
    if "T" not in _config1_cache:
        mesh, x, U, T0, bcs = config1_ref()
        ref = ScalarRef(mesh, "reduced", U, T0, bcs, c1.TAU, mu=c1.ALPHA)
        for _ in range(c1.STEPS):
            ref.step(c1.DT)
        _config1_cache["T"] = (x, ref.T)
    return _config1_cache["T"]


def test_restatement_meets_the_analytic_solution_of_config1():
    c1.check(*config1_restated())


def test_restatement_equals_the_banded_run_of_config1():
    import oracle
    from util import oracle_mesh_of

    def provider(mesh):
        om = oracle_mesh_of(mesh)
        return (lambda U, T, rho, tau_: oracle.qhd_fluxes(om, "reduced", U, T, rho, tau_, 0.0, (0, 0, 0))), np.full(mesh.nFaces, c1.TAU)
    x, T = c1.run(provider)
    x2, T2 = config1_restated()
    assert np.array_equal(x, x2) and np.abs(T - T2).max() <= 1e-12


def uniform_setup():
    mesh = make_mesh("box654_jitter")
    U, _ = smooth_fields(mesh)
    bcs = [{"U": ("zeroGradient", None), "T": ("zeroGradient", None)}] * mesh.nPatches
    return mesh, U, bcs, 300.0


def test_restatement_keeps_a_uniform_field_uniform():
    """div(phiTf) and Sp(div(phiu), T) cancel for a constant, whatever U is"""
    mesh, U, bcs, T0 = uniform_setup()
    ref = ScalarRef(mesh, "GaussVolPoint", U, np.full(mesh.nCells, T0), bcs, TAU, rho0=RHO0, mu=1e-2, Pr=PR)
    assert np.abs(ref.divPhiu).max() > 1e-4            # the velocity is not solenoidal: the Sp term is at work
    for _ in range(20):
        ref.step(1e-3)
    assert np.abs(ref.T - T0).max() <= 1e-12 * T0


# ---- CPU: reader / writer -----------------------------------------------------------------------------------------------------------------
def write_scalar_case(case_dir, stencil="GaussVolPoint", n=(6, 5, 4), qgd_extra="", div_line="", control_extra="", end_time=0.012, write_interval=6):
    mesh = q.PolyMesh.box(*n).jitter(0.1, seed=5)
    mesh.patch_names = ["inlet", "outlet", "wall", "top", "front", "back"]
    ff.write_polymesh(mesh, os.path.join(case_dir, "constant", "polyMesh"))
    U, T = smooth_fields(mesh)
    os.makedirs(os.path.join(case_dir, "system"), exist_ok=True)
    ff.write_field(os.path.join(case_dir, "0", "U"), mesh, "U", U,
                   {pn: (("fixedValue", np.array([1.1, 0.05, 0.0])) if pn == "inlet" else (("slip", None) if pn == "wall" else ("zeroGradient", None)))
                    for pn in mesh.patch_names}, "[0 1 -1 0 0 0 0]")
    ff.write_field(os.path.join(case_dir, "0", "T"), mesh, "T", T,
                   {pn: (("fixedValue", np.float64(1.3)) if pn == "inlet" else ("zeroGradient", None)) for pn in mesh.patch_names}, "[0 0 0 1 0 0 0]")
    with open(os.path.join(case_dir, "constant", "thermophysicalProperties"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="thermophysicalProperties") + textwrap.dedent(f'''
            thermoType {{ type heRhoQGDThermo; mixture pureMixture; transport const; thermo hConst;
                         equationOfState rhoConst; specie specie; energy sensibleInternalEnergy; }}
            mixture
            {{
                specie {{ molWeight 28.9; }}
                equationOfState {{ rho {RHO0}; }}
                thermodynamics {{ Cp 1005; Hf 0; }}
                transport {{ mu 1e-2; Pr {PR}; }}
            }}
            QGD
            {{
                {qgd_extra}
                QGDCoeffs constTau;
                constTauDict {{ Tau {TAU}; }}
            }}
            '''))
    with open(os.path.join(case_dir, "system", "fvSchemes"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="fvSchemes") + f"ddtSchemes {{ default Euler; }}\ngradSchemes {{ default Gauss linear; }}\n"
                f"divSchemes {{ default none; {div_line} }}\nlaplacianSchemes {{ default Gauss linear uncorrected; }}\n"
                f"interpolationSchemes {{ default linear; }}\nsnGradSchemes {{ default uncorrected; }}\nfvsc {{ default {stencil}; }}\n")
    with open(os.path.join(case_dir, "system", "fvSolution"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="fvSolution") + "solvers\n{\n    T { solver PBiCGStab; preconditioner DILU; tolerance 1e-12; relTol 0; maxIter 1500; }\n}\n")
    with open(os.path.join(case_dir, "system", "controlDict"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="controlDict") +
                f"application scalarTransportQHDFoam;\nstartFrom latestTime;\nstartTime 0;\nendTime {end_time};\ndeltaT 1e-3;\nwriteControl timeStep;\n"
                f"writeInterval {write_interval};\ntimePrecision 8;\n{control_extra}\n")
    return mesh, U, T


def test_read_scalar_case_setup(tmp_path):
    mesh, U, T = write_scalar_case(str(tmp_path))
    m2, opt, fields, bcs, control = ff.read_scalar_case_setup(str(tmp_path))
    assert m2.nCells == mesh.nCells and opt["stencil"] == "GaussVolPoint" and opt["deltaT"] == 1e-3 and opt["fluxSchemeT"] == 0
    assert opt["implicitDiffusion"] == 1 and opt["adjustTimeStep"] == 0 and "maxCo" not in opt     # the reference's default [QGDThermo.C L70-82]
    assert (opt["rho0"], opt["mu"], opt["Pr"]) == (RHO0, 1e-2, PR) and opt["tauModel"] == "constTau" and opt["Tau"] == TAU and opt["aQGD"] == 0.5
    assert (opt["implicitTol"], opt["implicitMaxIter"]) == (1e-12, 1500)
    assert control["endTime"] == 0.012 and control["writeInterval"] == 6
    by = dict(zip(m2.patch_names, bcs))
    assert by["inlet"]["T"] == ("fixedValue", 1.3) and by["inlet"]["U"][0] == "fixedValue" and tuple(by["inlet"]["U"][1]) == (1.1, 0.05, 0.0)
    assert by["wall"]["U"] == ("slip", None) and by["wall"]["T"] == ("zeroGradient", None) and by["outlet"]["T"] == ("zeroGradient", None)
    assert np.array_equal(fields["U"], U) and np.array_equal(fields["T"], T)
    # the other options
    d = tmp_path / "b"
    write_scalar_case(str(d), stencil="reduced", qgd_extra="implicitDiffusion false;", div_line="div(phiu,T) Gauss upwind;",
                      control_extra="adjustTimeStep yes;\nmaxCo 0.2;\nmaxDeltaT 0.5;\ncTau 0.6;")
    _, o, _, _, _ = ff.read_scalar_case_setup(str(d))
    assert o["stencil"] == "reduced" and o["implicitDiffusion"] == 0 and o["fluxSchemeT"] == 1
    assert o["adjustTimeStep"] == 1 and (o["maxCo"], o["maxDeltaT"], o["cTau"]) == (0.2, 0.5, 0.6)
    d = tmp_path / "c"
    write_scalar_case(str(d), control_extra="adjustTimeStep yes;\nmaxCo 0.2;")
    _, o, _, _, _ = ff.read_scalar_case_setup(str(d))
    assert o["cTau"] == 0.75 and o["maxDeltaT"] == 1e300


def test_scalar_reader_refuses_what_the_path_does_not_do(tmp_path):
    write_scalar_case(str(tmp_path))
    case = str(tmp_path)

    def refused(rel, old, new, match):
        path = os.path.join(case, rel)
        text = open(path).read()
        assert old in text
        open(path, "w").write(text.replace(old, new))
        with pytest.raises(ff.FoamFileError, match=match):
            ff.read_scalar_case_setup(case)
        open(path, "w").write(text)

    refused("constant/thermophysicalProperties", "QGDCoeffs constTau;", "QGDCoeffs constScPrModel1;", "closure")
    refused("constant/thermophysicalProperties", "equationOfState rhoConst;", "equationOfState perfectGas;", "rhoConst")
    refused("constant/thermophysicalProperties", "transport const;", "transport sutherland;", "thermoType.transport")
    refused("system/fvSchemes", "default none; ", "default none; div(phiu,T) Gauss vanLeer; ", r"div\(phiu,T\)")
    refused("system/fvSchemes", "Gauss linear uncorrected", "Gauss linear limited 0.5", "laplacianSchemes")
    refused("system/fvSchemes", "default Euler", "default backward", "ddtSchemes")
    refused("system/fvSchemes", "interpolationSchemes { default linear; }", "interpolationSchemes { default cubic; }", "interpolationSchemes")
    refused("0/T", "zeroGradient", "inletOutlet", "inletOutlet")
    ff.read_scalar_case_setup(case)   # and the untouched case still reads


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
PARITY = [("line1d", "reduced", 1e-2, False), ("line1d", "GaussVolPoint", 1e-2, False),
          ("plane2d_jitter", "GaussVolPoint", 1e-2, False), ("plane2d_jitter", "leastSquares", 1e-2, False),
          ("box654_jitter", "GaussVolPoint", 1e-2, False), ("box654_jitter", "reduced", 1e-2, False),
          ("box654_jitter", "GaussVolPoint", 0.0, False), ("plane2d_jitter", "GaussVolPoint", 1e-2, True),
          ("tet433", "GaussVolPoint", 1e-2, False), ("mix643", "reduced", 1e-2, False), ("prism543", "GaussVolPoint", 1e-2, True),
          ("ref533", "GaussVolPoint", 1e-2, False), ("ref533", "reduced", 1e-2, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,stencil,mu,upwind", PARITY)
def test_device_case_steps_like_the_restatement(kind, stencil, mu, upwind):
    mesh = make_mesh(kind)
    U, T = smooth_fields(mesh)
    bcs = mixed_bcs(mesh)
    ref = ScalarRef(mesh, stencil, U, T, bcs, TAU, rho0=RHO0, mu=mu, Pr=PR, upwind=upwind)
    dev, case = device_case(mesh, stencil, bcs, U, T, mu=mu, fluxSchemeT="upwind" if upwind else "linear")
    live = ref.live
    assert close(case.field("phiu")[live], ref.phiu[live], FLUX_TOL) and close(case.field("Uf")[live], ref.Uf[live], FLUX_TOL)
    assert np.array_equal(case.field("tauQGDf")[live], np.full(live.sum(), TAU))
    done = 0
    for chunk in (1, 9):
        case.step(chunk)
        for _ in range(chunk):
            ref.step(1e-3)
        done += chunk
        err = np.abs(case.field("T") - ref.T).max() / np.abs(ref.T).max()
        print(kind, stencil, mu, upwind, "steps", done, "T err", err, case.info())
        assert err <= T_TOL, (kind, stencil, done, err)
        assert close(case.field("T.boundary")[live[mesh.nInternalFaces:]], ref.Tb()[live[mesh.nInternalFaces:]], T_TOL)
        fl = ref.fluxes()
        for name in ("gradTf", "phiTauTReg", "phiTf"):
            a, b = case.field(name)[live], fl[name][live]
            e = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
            print("   ", name, e)
            # phiTf = phiu Tf is linear in T, which agrees to T_TOL after a solve: that is its bound once a step was made
            assert e <= (T_TOL if name == "phiTf" else FLUX_TOL), (name, e)
    info = case.info()
    assert info["steps"] == 10 and abs(info["time"] - 10e-3) <= 1e-15 and info["unconverged_steps"] == 0
    case.close(); dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,stencil", [("line1d", "reduced"), ("plane2d_jitter", "GaussVolPoint"), ("plane2d_jitter", "leastSquares"),
                                          ("box654_jitter", "GaussVolPoint"), ("tet433", "GaussVolPoint"), ("mix643", "GaussVolPoint")])
def test_device_face_fields_of_the_initial_state(kind, stencil):
    """before any solve the device and the restatement hold the same T bit for bit: phiu, phiTauTReg, gradTf to the face-field bound"""
    mesh = make_mesh(kind)
    U, T = smooth_fields(mesh)
    bcs = mixed_bcs(mesh)
    ref = ScalarRef(mesh, stencil, U, T, bcs, TAU, rho0=RHO0, mu=1e-2, Pr=PR)
    dev, case = device_case(mesh, stencil, bcs, U, T)
    assert np.array_equal(case.field("T"), T)
    fl = ref.fluxes()
    for name in ("phiu", "phiTauTReg", "gradTf", "phiTf"):
        a, b = case.field(name)[ref.live], fl[name][ref.live]
        e = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
        print(kind, stencil, name, e)
        assert e <= FLUX_TOL, (name, e)
    case.close(); dev.close()


@pytest.mark.gpu
def test_config1_resident_on_the_device():
    mesh, x, U, T0, bcs = config1_ref()
    dev, case = device_case(mesh, "reduced", bcs, U, T0, Tau=c1.TAU, rho0=1.0, Pr=1.0, mu=c1.ALPHA, deltaT=c1.DT)
    case.step(c1.STEPS)
    T = case.field("T")
    c1.check(x, T)
    x2, T2 = config1_restated()
    err = np.abs(T - T2).max() / np.abs(T2).max()
    print("config 1 device vs restatement", err, case.info())
    assert err <= T_TOL
    assert case.info()["steps"] == c1.STEPS
    case.close(); dev.close()


@pytest.mark.gpu
def test_device_keeps_a_uniform_field_uniform():
    mesh, U, bcs, T0 = uniform_setup()
    dev, case = device_case(mesh, "GaussVolPoint", bcs, U, np.full(mesh.nCells, T0))
    case.step(20)
    dev_err = np.abs(case.field("T") - T0).max() / T0
    print("uniform T after 20 steps", dev_err)
    assert dev_err <= 1e-12
    case.close(); dev.close()


@pytest.mark.gpu
def test_implicit_diffusion_false_leaves_T_as_listed():
    mesh = make_mesh("box654_jitter")
    U, T = smooth_fields(mesh)
    dev, case = device_case(mesh, "GaussVolPoint", mixed_bcs(mesh), U, T, implicitDiffusion=0)
    case.step(5)
    info = case.info()
    assert np.array_equal(case.field("T"), T) and info["steps"] == 5 and abs(info["time"] - 5e-3) <= 1e-15 and info["solver"] is None
    case.close(); dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dt0", [5e-3, 1e-5])
def test_adjust_time_step_follows_the_listing(dt0):
    mesh = make_mesh("box654_jitter")
    U, T = smooth_fields(mesh)
    bcs = mixed_bcs(mesh)
    max_co, max_dt, c_tau = 5e-3, 1.0, 0.75
    dev, case = device_case(mesh, "GaussVolPoint", bcs, U, T, deltaT=dt0, adjustTimeStep=1, maxCo=max_co, maxDeltaT=max_dt, cTau=c_tau)
    ref = ScalarRef(mesh, "GaussVolPoint", U, T, bcs, TAU, rho0=RHO0, mu=1e-2, Pr=PR)
    h, Uf, tau = case.field("hQGDf"), case.field("Uf"), case.field("tauQGDf")
    live = ref.live
    max_ubyh = (np.sqrt((Uf[live] ** 2).sum(axis=1)) / h[live]).max()
    dt, dts = dt0, []
    for step in range(12):
        co, dt_new = delta_t_rule(dt, max_ubyh, tau[live].min(), max_co, max_dt, c_tau)
        case.step(1)
        info = case.info()
        print("step", step, "deltaT", info["deltaT"], dt_new, "CoNum", info["CoNum"], co)
        assert abs(info["deltaT"] - dt_new) <= 1e-14 * dt_new
        assert abs(info["CoNum"] - dt * max_ubyh) <= 1e-13 * co
        dt = info["deltaT"]
        dts.append(dt)
        ref.step(dt)
    assert (dts[-1] < 0.5 * dt0) if dt0 > 1e-3 else (dts[-1] > 2.0 * dt0)      # the control did act, in the direction the start value asks for
    assert abs(case.info()["time"] - sum(dts)) <= 1e-13 * sum(dts)
    err = np.abs(case.field("T") - ref.T).max() / np.abs(ref.T).max()
    print("T err", err)
    assert err <= T_TOL
    case.close(); dev.close()


@pytest.mark.gpu
def test_solver_statistics(monkeypatch):
    mesh = make_mesh("box654_jitter")
    U, T = smooth_fields(mesh)
    bcs = mixed_bcs(mesh)
    dev, case = device_case(mesh, "GaussVolPoint", bcs, U, T, implicitTol=1e-10, implicitMaxIter=500)
    case.step(3)
    info = case.info()
    print(info)
    assert 0 < info["iterations"] < 500 and info["finalResidual"] < 1e-10 and info["initialResidual"] > info["finalResidual"]
    assert info["unconverged_steps"] == 0 and info["solver"] == "chebyshev"
    T_cheb = case.field("T")
    case.close()
    # an iteration limit of one under a tolerance nothing reaches: every step is counted, T stays finite
    from qgdsolver_amd import scalarfoam
    c2 = scalarfoam.ScalarTransportQHDCase(dev, scalarfoam.scalar_options(stencil="GaussVolPoint", tauModel="constTau", Tau=TAU, rho0=RHO0, Pr=PR, mu=1e-2,
                                                                           deltaT=1e-3, implicitTol=1e-300, implicitMaxIter=1))
    for i, bc in enumerate(bcs):
        c2.set_bc(i, U=bc["U"], T=bc["T"])
    c2.set_fields(U, T)
    c2.step(4)
    i2 = c2.info()
    assert i2["unconverged_steps"] == 4 and i2["steps"] == 4 and np.isfinite(c2.field("T")).all()
    c2.close()
    # conjugate gradients instead of the Chebyshev iteration: the same T
    monkeypatch.setenv("QGD_IMPL_SOLVER", "pcg")
    dev3, c3 = device_case(mesh, "GaussVolPoint", bcs, U, T, implicitTol=1e-13, implicitMaxIter=500)
    c3.step(3)
    assert c3.info()["solver"] == "pcg" and close(c3.field("T"), T_cheb, T_TOL)
    c3.close(); dev3.close(); dev.close()


@pytest.mark.gpu
def test_refusals():
    from qgdsolver_amd import scalarfoam
    from qhd_shards import box_slabs
    sh = box_slabs(6, 5, 12, 2)[0]
    dev = q.Device(sh["mesh"], fused_tables=False)
    with pytest.raises(q.QgdError, match="sharded") as e:
        scalarfoam.ScalarTransportQHDCase(dev, scalarfoam.scalar_options())
    assert e.value.code == L.ERR_NOT_IMPLEMENTED
    dev.close()
    G, CYC = L.PATCH_GENERIC, L.PATCH_CYCLIC
    ext = q.PolyMesh.box(6, 5, 4, patch_types=[CYC, CYC, G, G, G, G]).unroll_cyclic()
    dev = q.Device(ext, fused_tables=False)
    with pytest.raises(q.QgdError, match="unrolled") as e:
        scalarfoam.ScalarTransportQHDCase(dev, scalarfoam.scalar_options())
    assert e.value.code == L.ERR_NOT_IMPLEMENTED
    dev.close()
    mesh = make_mesh("box654")
    U, T = smooth_fields(mesh)
    dev, case = device_case(mesh, "GaussVolPoint", mixed_bcs(mesh), U, T)
    with pytest.raises(q.QgdError) as e:
        case.set_bc(0, T=("inletOutlet", None))
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(q.QgdError) as e:
        case.set_bc(0, U=("noSlipish", None))
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(q.QgdError) as e:
        case.field("p")
    assert e.value.code == L.ERR_INVALID
    case.close(); dev.close()


@pytest.mark.gpu
def test_symmetry_plane_behaves_as_a_slip_wall():
    """a symmetryPlane patch keeps its own field types whatever is asked for: slip for U, zeroGradient for T"""
    mesh = make_mesh("box_sym")
    U, T = smooth_fields(mesh)
    bcs = mixed_bcs(mesh)
    bcs[2] = {"U": ("fixedValue", (9.0, 9.0, 9.0)), "T": ("fixedValue", 9.0)}      # ignored on the constraint patch
    ref = ScalarRef(mesh, "GaussVolPoint", U, T, bcs, TAU, rho0=RHO0, mu=1e-2, Pr=PR)
    dev, case = device_case(mesh, "GaussVolPoint", bcs, U, T)
    assert close(case.field("phiu")[ref.live], ref.phiu[ref.live], FLUX_TOL)
    case.step(5)
    for _ in range(5):
        ref.step(1e-3)
    assert close(case.field("T"), ref.T, T_TOL)
    case.close(); dev.close()


@pytest.mark.gpu
def test_case_left_open_is_freed_by_its_device():
    mesh = make_mesh("box654")
    U, T = smooth_fields(mesh)
    dev, case = device_case(mesh, "GaussVolPoint", mixed_bcs(mesh), U, T)
    case.step(1)
    rc = L.lib.qgd_device_free(dev._h)                 # the C-ABI's own guard
    assert rc != L.QGD_OK and b"still open" in L.lib.qgd_last_error()
    dev.close()                                        # frees the adopted case first
    assert dev._h is None and case._h is None
    case.close()                                       # idempotent


@pytest.mark.gpu
def test_application_round_trip_and_restart(tmp_path):
    full, half = str(tmp_path / "full"), str(tmp_path / "half")
    mesh, U, T = write_scalar_case(full)
    write_scalar_case(half, end_time=0.006)
    app = [sys.executable, "-m", "qgdsolver_amd.scalarTransportQHDFoam", "-case"]
    pr = subprocess.run(app + [full], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-1500:]
    out = pr.stdout
    assert "Courant Number max:" in out and "deltaT = 0.001" in out and "max/min of T" in out and "Time = 0.012" in out and out.rstrip().endswith("End")
    assert "WARNING" not in out and "Solving for T" in out
    assert sorted(d for d in os.listdir(full) if d[0].isdigit()) == ["0", "0.006", "0.012"]
    assert sorted(os.listdir(os.path.join(full, "0.012"))) == ["T", "U", "rho"]
    # stopped halfway, then restarted from its latest time directory: bit for bit the uninterrupted run
    pr = subprocess.run(app + [half], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-1500:]
    assert sorted(d for d in os.listdir(half) if d[0].isdigit()) == ["0", "0.006"]
    cd = os.path.join(half, "system", "controlDict")
    text = open(cd).read()
    open(cd, "w").write(text.replace("endTime 0.006;", "endTime 0.012;"))
    pr = subprocess.run(app + [half], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-1500:]
    assert "start 0.006" in pr.stdout
    m2 = ff.read_polymesh(os.path.join(full, "constant", "polyMesh"))
    a, pa = ff.read_field(os.path.join(full, "0.012", "T"), m2)
    b, _ = ff.read_field(os.path.join(half, "0.012", "T"), m2)
    assert np.array_equal(a, b)
    assert pa["inlet"]["type"] == "fixedValue" and np.all(pa["inlet"]["value"] == 1.3)
    ua, _ = ff.read_field(os.path.join(full, "0.012", "U"), m2)
    assert np.array_equal(ua, U)
    # and equal to the restatement
    ref = ScalarRef(mesh, "GaussVolPoint", U, T, [{"U": ("fixedValue", (1.1, 0.05, 0.0)), "T": ("fixedValue", 1.3)}, {"U": ("zeroGradient", None), "T": ("zeroGradient", None)},
                                                 {"U": ("slip", None), "T": ("zeroGradient", None)}] + [{"U": ("zeroGradient", None), "T": ("zeroGradient", None)}] * 3,
                    TAU, rho0=RHO0, mu=1e-2, Pr=PR)
    for _ in range(12):
        ref.step(1e-3)
    assert close(a[:, 0], ref.T, 1e-9)                 # the case's fvSolution tolerance is 1e-12, as in tests/test_qhdfoam_case.py
    # implicitDiffusion false: the application says what the listing does
    off = str(tmp_path / "off")
    write_scalar_case(off, qgd_extra="implicitDiffusion false;", end_time=0.002, write_interval=2)
    pr = subprocess.run(app + [off], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert pr.returncode == 0 and pr.stdout.count("WARNING") == 1 and "no else" in pr.stdout.replace("\n", " ")
