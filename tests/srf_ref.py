"""Reference for one step of the rotating-frame QHD case (SRFQHDFoam), built from steps of the CPU oracle, which knows QHDFoam's
body force beta*T*g only.

One QHD step from a given (U, T, p) is AFFINE in the body-force field B (cells and patch values): B enters phiwo linearly, the
pressure equation is linear with a right-hand side linear in phiwo, Wf and the U equation are linear in B, p and phi (linear
qgdFlux; U, T, p of the start of the step are data).  So step(B) = step(0) + L(B), and with

    B_SRF = beta*T*g + sum_k U_k a_k,        a_k = -2 (omega ^ e_k)      [SRFQHDFoam/updateFields.H L73]

    step_SRF = step_oracle(beta, g, T) + sum_{k=0..2} step_oracle(beta = 1, g = a_k, T = U_k) - 3 step_oracle(beta = 0)

for U, p, phi and their patch values after ONE step (the oracle's own T equation does not reach them within the step).  Run k
carries U_k as its temperature, so its T boundary condition mirrors U's: the patch value of B is the same expression on the
patch values.  fixedValue U -> fixedValue T with (U_b)_k; zeroGradient -> zeroGradient; slip (flat, axis-aligned faces only) ->
zeroGradient for a tangential k, fixedValue 0 for the normal k; empty -> none.
With beta*T*g = 0 the first and the last term cancel to the issue's form sum_k step_k - 2 step(T = 0).
"""
import os
import textwrap

import numpy as np

import qgdsolver_amd as q
from qgdsolver_amd import foamfile as ff, qhdfoam

from oracle import OracleQhdCase
from util import oracle_mesh_of

OMEGA_3D = np.array([3.0, -4.0, 4.4])      # oblique, |omega| = 6.66 rad/s
OMEGA_2D = np.array([0.0, 0.0, 6.7])       # along the empty direction of plane2d / plane2d_jitter
INLET = np.array([0.3, 0.05, -0.02])
FIELDS = ("U", "p", "phi", "U.boundary", "p.boundary")


def options(stencil="GaussVolPoint", implicit=0, **kw):
    base = dict(stencil=stencil, tauModel="HbyUQHD", aQGD=0.5, UQHD=1.0, rho0=1.0, mu=1e-2, Pr=0.71, beta=3e-3, g=(0.0, -9.81, 0.0),
                deltaT=2e-3, pTol=1e-13, pMaxIter=3000, pRefCell=0, pRefValue=0.0, precond=1, implicitDiffusion=implicit,
                implicitTol=1e-12, implicitMaxIter=2000)
    base.update(kw)
    return qhdfoam.qhd_options(**base)


def copy_options(opt, **kw):
    o = type(opt)()
    for f, _ in opt._fields_:
        v = getattr(opt, f)
        if f == "g":
            for k in range(3):
                o.g[k] = v[k]
        else:
            setattr(o, f, v)
    for k, v in kw.items():
        if k == "g":
            for i in range(3):
                o.g[i] = float(v[i])
        else:
            setattr(o, k, v)
    return o


def patch_bcs(mesh, slip=False):
    """per patch (U, T, p): fixedValue inlet with p zeroGradient (patch 0), zeroGradient outlet with p fixedValue (patch 1), no-slip walls
    with qhdFluxCoupled; slip: patches 2, 3 are slip walls with p zeroGradient; empty patches carry nothing"""
    types = mesh.array("patchType")
    inlet = INLET.copy()
    if mesh.nGeometricD == 2:
        inlet[2] = 0.0
    out = []
    for ip in range(mesh.nPatches):
        if types[ip] == q._lib.PATCH_EMPTY:
            out.append(dict(U=("none", None), T=("none", None), p=("none", None)))
        elif ip == 0:
            out.append(dict(U=("fixedValue", tuple(inlet)), T=("fixedValue", 305.0), p=("zeroGradient", None)))
        elif ip == 1:
            out.append(dict(U=("zeroGradient", None), T=("zeroGradient", None), p=("fixedValue", 0.0)))
        elif slip and ip in (2, 3):
            out.append(dict(U=("slip", None), T=("zeroGradient", None), p=("zeroGradient", None)))
        else:
            out.append(dict(U=("fixedValue", (0.0, 0.0, 0.0)), T=("zeroGradient", None), p=("qhdFluxCoupled", None)))
    return out


def initial(mesh, seed=5):
    C = mesh.array("C").reshape(-1, 3)
    rng = np.random.default_rng(seed)
    inlet = INLET.copy()
    U = inlet + 0.2 * rng.standard_normal((mesh.nCells, 3))
    if mesh.nGeometricD == 2:
        U[:, 2] = 0.0
    return U, 300.0 + 10.0 * (0.5 - C[:, 0]), 0.1 * rng.standard_normal(mesh.nCells)


def apply_bcs(case, bcs):
    for ip, bc in enumerate(bcs):
        case.set_bc(ip, U=bc["U"], T=bc["T"], p=bc["p"])


class SrfReference:
    """the five oracle cases of the superposition on one mesh; step(U, T, p) -> the fields after one rotating-frame step"""

    def __init__(self, mesh, opt, bcs, omega):
        om = oracle_mesh_of(mesh)
        self.mesh = mesh
        omega = np.asarray(omega, dtype=np.float64)
        buoy = OracleQhdCase(om, opt)
        apply_bcs(buoy, bcs)
        self.buoy = buoy
        zero = OracleQhdCase(om, copy_options(opt, beta=0.0))
        apply_bcs(zero, bcs)
        self.zero = zero
        self.comp = []
        for k in range(3):
            a = -2.0 * np.cross(omega, np.eye(3)[k])
            c = OracleQhdCase(om, copy_options(opt, beta=1.0, g=a))
            for ip, bc in enumerate(bcs):
                kind, val = bc["U"]
                if kind == "fixedValue":
                    tb = ("fixedValue", float(val[k]))
                elif kind == "slip":
                    tb = ("fixedValue", 0.0) if k == ip // 2 else ("zeroGradient", None)   # PolyMesh.box: patches 2a, 2a+1 are normal to axis a
                else:
                    tb = (kind, None)
                c.set_bc(ip, U=bc["U"], T=tb, p=bc["p"])
            self.comp.append(c)

    def step(self, U, T, p):
        """-> (fields of the rotating-frame step, fields of the step without the Coriolis force)"""
        def one(case, temp):
            case.set_fields(U, temp, p)
            case.step(1)
            return {f: case.field(f) for f in FIELDS}
        b, z = one(self.buoy, T), one(self.zero, T)
        ks = [one(c, np.ascontiguousarray(U[:, k])) for k, c in enumerate(self.comp)]
        return {f: b[f] + ks[0][f] + ks[1][f] + ks[2][f] - 3.0 * z[f] for f in FIELDS}, b

    def close(self):
        for c in [self.buoy, self.zero] + self.comp:
            c.close()


def rel(a, ref):
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


HDR = "FoamFile {{ version 2.0; format ascii; class {cls}; object {obj}; }}\n"


def write_srf_case(case_dir, n=(6, 5, 4), rpm=60.0, axis=(0, 0, 2), origin=(0.5, 0.5, 0.0), urel_entries=None, srf_text=None,
                   velocity_file="Urel", implicit_line="implicitDiffusion false;"):
    """a small rotating box: `casing` (xMin) at rest in the inertial frame (SRFVelocity, relative no), `rotor` (xMax) a no-slip wall that
    turns with the frame, the other walls no-slip in the frame as well"""
    mesh = q.PolyMesh.box(*n).jitter(0.1, seed=7)
    mesh.patch_names = ["casing", "rotor", "floor", "ceiling", "front", "back"]
    ff.write_polymesh(mesh, os.path.join(case_dir, "constant", "polyMesh"))

    def bf(entries):
        return "boundaryField\n{\n" + "\n".join(f"    {n} {{ {entries.get(n, entries['default'])} }}" for n in mesh.patch_names) + "\n}\n"

    os.makedirs(os.path.join(case_dir, "0"))
    os.makedirs(os.path.join(case_dir, "system"))
    entries = {"casing": "type SRFVelocity; relative no; inletValue uniform (0 0 0); value uniform (0 0 0);",
               "default": "type fixedValue; value uniform (0 0 0);"}
    entries.update(urel_entries or {})
    with open(os.path.join(case_dir, "0", velocity_file), "w") as f:
        f.write(HDR.format(cls="volVectorField", obj=velocity_file) + "dimensions [0 1 -1 0 0 0 0];\ninternalField uniform (0 0 0);\n" + bf(entries))
    with open(os.path.join(case_dir, "0", "T"), "w") as f:
        f.write(HDR.format(cls="volScalarField", obj="T") + "dimensions [0 0 0 1 0 0 0];\ninternalField uniform 300;\n" +
                bf({"default": "type zeroGradient;"}))
    with open(os.path.join(case_dir, "0", "p"), "w") as f:
        f.write(HDR.format(cls="volScalarField", obj="p") + "dimensions [0 2 -2 0 0 0 0];\ninternalField uniform 0;\n" +
                bf({"default": "type qhdFlux;"}))
    with open(os.path.join(case_dir, "constant", "SRFProperties"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="SRFProperties") +
                (srf_text if srf_text is not None else
                 f"SRFModel rpm;\norigin ({origin[0]} {origin[1]} {origin[2]});\naxis ({axis[0]} {axis[1]} {axis[2]});\nrpmCoeffs {{ rpm {rpm}; }}\n"))
    with open(os.path.join(case_dir, "constant", "thermophysicalProperties"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="thermophysicalProperties") + textwrap.dedent(f'''
            thermoType {{ type heRhoQGDThermo; mixture pureMixture; transport const; thermo hConst;
                         equationOfState rhoConst; specie specie; energy sensibleInternalEnergy; }}
            mixture
            {{
                specie {{ molWeight 28.9; }}
                equationOfState {{ rho 1.2; }}
                thermodynamics {{ Cp 1005; Hf 0; }}
                transport {{ mu 1.8e-2; Pr 0.71; beta 0; }}
            }}
            QGD
            {{
                {implicit_line}
                QGDCoeffs HbyUQHD;
                HbyUQHDDict {{ UQHD 0.8; }}
                pRefCell 17;
                pRefValue 0.25;
            }}
            '''))
    with open(os.path.join(case_dir, "constant", "gravitationalProperties"), "w") as f:
        f.write(HDR.format(cls="uniformDimensionedVectorField", obj="gravitationalProperties") + "g g [0 1 -2 0 0 0 0] (0 0 0);\n")
    with open(os.path.join(case_dir, "system", "fvSchemes"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="fvSchemes") + "ddtSchemes { default Euler; }\ngradSchemes { default Gauss linear; }\n"
                "divSchemes { default none; }\nlaplacianSchemes { default Gauss linear uncorrected; }\n"
                "interpolationSchemes { default linear; }\nsnGradSchemes { default corrected; }\nfvsc { default GaussVolPoint; }\n")
    with open(os.path.join(case_dir, "system", "fvSolution"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="fvSolution") + textwrap.dedent('''
            solvers
            {
                p { solver PCG; preconditioner DIC; tolerance 1e-12; relTol 0; maxIter 2000; }
                "(U|T)" { solver PBiCGStab; preconditioner DILU; tolerance 1e-12; relTol 0; maxIter 1500; }
            }
            '''))
    with open(os.path.join(case_dir, "system", "controlDict"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="controlDict") +
                "application SRFQHDFoam;\nstartFrom latestTime;\nstartTime 0;\nendTime 0.006;\ndeltaT 1e-3;\nwriteControl timeStep;\nwriteInterval 3;\n"
                "timePrecision 8;\n")
    return mesh
