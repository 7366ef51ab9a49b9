"""GPU: the pressure preconditioner z = M r (one multigrid V-cycle, qgd_poisson.hip) as an operator, against the numpy replay of
tests/mg_ref.py fed with the arrays the DEVICE holds (QHDFoamCase.mg_info / mg_level / mg_apply).

A preconditioner that is subtly wrong still lets CG converge, only more slowly, so the converged pressure cannot pin it.  Here:
 (a) the stored hierarchy is what the comments say (symmetric levels, P^T the transpose of P, Galerkin coarse operators, inverse, scales);
 (b) one application on the device equals the replay (double cycle: 1e-10; single-precision cycle: 4 x the replay's own float32 error);
 (c) the cycle is the symmetric positive (semi-)definite operator CG needs;
 (d) the three entries change no bit of a run.
Meshes of one to a few thousand cells; QGD_MG_DENSE_MAX=64 forces deep hierarchies on them.

kernel -> rows of ROWS whose (b) / (c) assertions run it (test_one_application_matches_the_replay and the others take every row):
  mgSmoothKernel<float>        every single-precision row (level 0)          <double>  every 'double ...' row
  mgSmoothRowKernel<float>     hex ragged, polyhedra (CSR-rows levels)       <double>  double polyhedra
  mgSmoothLastKernel           test_fused_tail_is_the_separate_passes (every row with a fused hand-over; float only)
  mgConvertKernel              every single-precision row (both directions; float -> double not in the tail mode; no double cycle uses it)
  mgRestrictRowKernel<float>   every smoothed row but 'sliced transpose'     <double>  double hex, double polyhedra, double singular ...
  mgRestrictEllKernel<float>   sliced transpose                              <double>  double sliced transpose
  mgProlongEllKernel<float>    every smoothed row                            <double>  every smoothed 'double ...' row
  mgRestrictKernel / mgProlongKernel<float>   plain, plain one pass          <double>  double plain
  mgDenseKernel<float>         every row with a dense last level             <double>  double hex, double polyhedra, double sliced transpose, double plain
  mgCoarseKernel<float>        singular, singular deep, singular wide (rows of 37 entries: past the 32 it keeps in registers)
                                                                             <double>  double singular deep
  sweep loop on the last level mgSmoothKernel: singular ragged (2035 rows);  mgSmoothRowKernel: singular polyhedra, <double> double singular polyhedra
(test_row_has_the_structure_its_checks_need and test_every_layout_occurs assert the layouts behind this table, so a change of the builder's
thresholds cannot empty a line silently.)

The 'singular' rows have all-Neumann pressure patches and no reference cell.  Only where the builder coarsens down to a last level and its
Cholesky factorisation then fails (singular deep, singular wide, singular polyhedra and their double rows) is that the fallback from a failed
dense inverse; the one-level rows 'singular' and 'singular ragged' reach the last-level Jacobi sweeps simply because level 0 is never
inverted (default QGD_MG_DENSE_MAX, at most 2048 cells), whatever pRefCell is."""
import contextlib
import os

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd import qhdfoam
from qgdsolver_amd.synthetic import c5_mesh

import mg_ref
from test_qhd_case import cavity_bcs, initial, options
from util import make_mesh

pytestmark = pytest.mark.gpu

G, E = L.PATCH_GENERIC, L.PATCH_EMPTY
DEEP = {"QGD_MG_DENSE_MAX": "64"}
MESHES = {
    "hex": lambda: q.PolyMesh.box(12, 10, 8).jitter(0.15, seed=5),                                   # 960 cells
    "hex880": lambda: q.PolyMesh.box(11, 10, 8).jitter(0.15, seed=5),                                # a single level of it is no multiple of 64
    "ragged": lambda: q.PolyMesh.box(37, 11, 5),                                                     # 2035: tiles and slices end ragged
    "2d": lambda: q.PolyMesh.box(40, 30, 1, hi=(1.0, 0.75, 0.025), patch_types=[G, G, G, G, E, E]).jitter(0.15, seed=11),
    "chain": lambda: q.PolyMesh.box(1024, 1, 1, hi=(1.0, 0.001, 0.001), patch_types=[G, G, E, E, E, E]),   # rows of width <= 2
    "polyhedra": lambda: c5_mesh(16, 8 ** 3, poly=True),
    "plain": lambda: q.PolyMesh.box(20, 14, 9),                                                      # 2520 -> 630 -> 157
    "tetrahedra": lambda: make_mesh("tet866"),                                                       # 1728 rows of <= 4 entries: 1728 -> 313 -> 22
    "refined": lambda: make_mesh("ref533"),                                                          # 143 rows of 6 to 24 entries beside each other
}
# tag: (mesh, knobs, all-Neumann pressure without a reference cell)
ROWS = {
    "hex": ("hex", DEEP, False),
    "hex ragged": ("ragged", DEEP, False),
    "2d": ("2d", DEEP, False),
    "chain": ("chain", DEEP, False),
    "polyhedra": ("polyhedra", DEEP, False),
    "sliced transpose": ("hex", dict(DEEP, QGD_MG_PT_ELL_MIN="0"), False),
    "double hex": ("hex", dict(DEEP, QGD_MG_F32="0"), False),
    "double polyhedra": ("polyhedra", dict(DEEP, QGD_MG_F32="0"), False),
    "chebyshev": ("hex", dict(DEEP, QGD_MG_CHEB="10", QGD_MG_NU="3"), False),
    "nu0": ("hex", dict(DEEP, QGD_MG_NU0="1"), False),
    "plain": ("plain", {"QGD_MG_SA": "0"}, False),
    "plain one pass": ("plain", {"QGD_MG_SA": "0", "QGD_MG_PASSES": "1"}, False),
    "singular": ("hex880", {}, True),
    "singular deep": ("hex", DEEP, True),
    "singular ragged": ("ragged", {}, True),
    "singular wide": ("hex", {"QGD_MG_DENSE_MAX": "128"}, True),                      # 960 -> 124 rows of up to 37 entries, no inverse
    "singular polyhedra": ("polyhedra", {}, True),                                    # 4096 -> 490 CSR rows, no inverse
    "double sliced transpose": ("hex", dict(DEEP, QGD_MG_F32="0", QGD_MG_PT_ELL_MIN="0"), False),
    "double plain": ("plain", {"QGD_MG_SA": "0", "QGD_MG_F32": "0"}, False),
    "double singular deep": ("hex", dict(DEEP, QGD_MG_F32="0"), True),
    "double singular polyhedra": ("polyhedra", {"QGD_MG_F32": "0"}, True),
    # a graph no box of hexahedra has: four neighbours per cell at most, aggregates grown over 24 cells per vertex (tests/unstructured.py)
    "tetrahedra": ("tetrahedra", DEEP, False),
    "double tetrahedra": ("tetrahedra", dict(DEEP, QGD_MG_F32="0"), False),
    # one level of 2:1 refinement (tests/unstructured.py): a coarse cell between refined ones has 24 neighbours, its children's cells six -- the
    # row walks of the level-0 sweeps take three passes of eight on some lanes of a wavefront and one on the others
    "refined": ("refined", DEEP, False),
    "double refined": ("refined", dict(DEEP, QGD_MG_F32="0"), False),
}
FEW_LEVELS = {"singular": 1, "singular ragged": 1, "singular wide": 2, "singular polyhedra": 2, "double singular polyhedra": 2,
              "refined": 2, "double refined": 2}           # 143 rows: one coarsening reaches the dense last level
SWEEP_LOOP = {"singular ragged": "ell", "singular polyhedra": "csr", "double singular polyhedra": "csr"}     # else mgCoarseKernel
DEFAULT_ROWS = ("hex", "hex ragged", "2d", "chain", "polyhedra")
MG_KNOBS = ("QGD_MG_DIST", "QGD_MG_DENSE_MAX", "QGD_MG_PT_ELL_MIN", "QGD_MG_F32", "QGD_MG_CHEB", "QGD_MG_NU", "QGD_MG_NU0", "QGD_MG_SA", "QGD_MG_PASSES",
            "QGD_MG_FUSE", "QGD_MG_OC", "QGD_MG_OMEGA", "QGD_MG_COARSE_SWEEPS", "QGD_MG_CHEB_LMAX", "QGD_MG_SA_THETA")


@contextlib.contextmanager
def knobs(env):
    """the solver reads its knobs when set_fields creates it"""
    old = {k: os.environ.get(k) for k in MG_KNOBS}
    try:
        for k in MG_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Observed:
    def __init__(self, tag, case, mesh):
        self.tag, self.case, self.mesh = tag, case, mesh
        self.info = case.mg_info()
        self.arrays = [case.mg_level(l) for l in range(len(self.info["levels"]))]
        self.cycle = mg_ref.Cycle.from_case_arrays(self.info, self.arrays)
        self.n = self.info["levels"][0]["n"]
        self.dt = np.float32 if self.info["f32"] else np.float64
        self.singular = ROWS[tag][2]

    def shape(self):
        return " -> ".join(f"{m['n']}{'c' if m['layout'] == 'csr' else 'e'}{'D' if m['dense'] else ''}{'t' if m['ptSliced'] else ''}"
                           for m in self.info["levels"])


@contextlib.contextmanager
def observe(tag):
    kind, env, neumann = ROWS[tag]
    mesh = MESHES[kind]()
    dev = q.Device(mesh)
    with knobs(env):
        case = qhdfoam.QHDFoamCase(dev, options(deltaT=1e-3, pTol=1e-10, pRefCell=-1 if neumann else 0))
        cavity_bcs(case, mesh)
        case.set_fields(*initial(mesh))
    try:
        yield Observed(tag, case, mesh)
    finally:
        case.close(); dev.close()


@pytest.fixture(scope="module", params=list(ROWS))
def row(request):
    with observe(request.param) as o:
        yield o


def inputs(o):
    """random r and the unit vectors at row 0, at the last row and at the first row of the last slice of 64"""
    n = o.n
    out = [("random", np.random.default_rng(7).standard_normal(n))]
    for name, i in (("e_0", 0), ("e_last", n - 1), ("e_last_slice", (n - 1) // 64 * 64)):
        e = np.zeros(n); e[i] = 1.0
        out.append((name, e))
    return out


def dense_of(level):
    A = np.diag(level.diag.astype(np.float64))
    np.subtract.at(A, (level.A[0], level.A[1]), level.A[2].astype(np.float64))
    return A


def double_level(a, m):
    """(diag, (row, col, a_ij)) of the double-precision arrays of a level, dense A of them on request"""
    dec = mg_ref.decode_csr if m["layout"] == "csr" else mg_ref.decode_ell
    return a["diag64"], dec(a["start"], a["col"], a["val64"], m["n"])


def dense_double(a, m):
    d, (r, c, v) = double_level(a, m)
    A = np.diag(d)
    np.subtract.at(A, (r, c), v)
    return A


def localise(o, r):
    """where a mismatch of the whole cycle would come from: per level and stage, the distance between the replay as stored and the replay
    with the reference inverse on the last level (a float64 solve with the decoded matrix) / with P transposed in place of the stored P^T"""
    base, exact, transposed = {}, {}, {}
    o.cycle.apply(r, o.dt, trace=base)
    o.cycle.apply(r, o.dt, trace=exact, exact_last=True)
    o.cycle.apply(r, o.dt, trace=transposed, stored_transpose=False)
    lines = []
    for l in sorted(base):
        for st in mg_ref.STAGES:
            if st in base[l]:
                s = max(np.abs(base[l][st]).max(), 1e-300)
                lines.append(f"  level {l} {st:10s} |stored - reference inverse| = {np.abs(base[l][st] - exact[l][st]).max() / s:.2e}"
                             f"   |stored P^T - transposed P| = {np.abs(base[l][st] - transposed[l][st]).max() / s:.2e}")
    return "\n".join(lines)


# ---- structure ------------------------------------------------------------------------------------------------------------------------
def test_row_has_the_structure_its_checks_need(row):
    o, lv = row, row.info["levels"]
    print(f"PARITY {o.tag}: levels {o.shape()}  f32={o.info['f32']} sa={o.info['sa']} nu={o.info['nu']} nu0={o.info['nu0']} fused={o.info['fused']}")
    if o.tag in FEW_LEVELS:
        assert len(lv) == FEW_LEVELS[o.tag], o.shape()
    else:
        assert len(lv) >= 3, o.shape()
    assert any(m["n"] % 64 for m in lv), o.shape()
    widths = []
    for a, m in zip(o.arrays, lv):
        if m["layout"] == "ell":
            widths += list(np.diff(a["start"][:(m["n"] + 63) // 64 + 1]))
        if "pS" in a:
            widths += list(np.diff(a["pS"][:(m["n"] + 63) // 64 + 1]))
    assert any(w % 8 for w in widths), (o.tag, sorted(set(widths)))
    if "sliced transpose" in o.tag:
        assert all(m["ptSliced"] and m["smoothed"] for m in lv[:-1]) and o.info["ptEllMin"] == 0, lv
    elif o.info["sa"]:
        assert not any(m["ptSliced"] for m in lv) and o.info["ptEllMin"] == 300000, lv
    if "plain" in o.tag:
        assert not o.info["sa"] and all("pS" not in a for a in o.arrays) and all("agg" in a for a in o.arrays[:-1])
    if o.tag.startswith("double"):
        assert not o.info["f32"] and not o.info["fused"]
    else:
        assert o.info["f32"]
    if o.tag == "chebyshev":
        assert o.info["nu"] == 3 and np.all(o.info["cm"][1:] > 0) and o.info["cr"][0] != o.info["omega"]
    if o.tag == "nu0":
        assert o.info["nu0"] == 1 and o.info["nu"] == 2
    if o.singular:
        last = lv[-1]
        assert not last["dense"] and "inverse" not in o.arrays[-1], last
        coarse_kernel = last["layout"] == "ell" and last["n"] <= 1024          # mgCoarseKernel; otherwise the generic sweep loop
        assert coarse_kernel == (o.tag not in SWEEP_LOOP) and (coarse_kernel or last["layout"] == SWEEP_LOOP[o.tag]), (o.tag, last)
        if o.tag == "singular wide":
            assert last["width"] > 32 and np.diff(o.arrays[-1]["start"][:2])[0] > 32, last
    else:
        assert lv[-1]["dense"] and o.arrays[-1]["inverse"].size == lv[-1]["n"] ** 2, lv[-1]


def test_every_layout_occurs():
    """across the default rows: a sliced-ELL level below level 0, a CSR-rows level, a CSR P^T and a dense last level"""
    seen = set()
    for tag in DEFAULT_ROWS:
        with observe(tag) as o:
            lv = o.info["levels"]
            seen |= {f"{m['layout']} below 0" for m in lv[1:]}
            seen |= {"csr transpose" for m in lv[:-1] if m["smoothed"] and not m["ptSliced"]}
            seen |= {"dense last" for m in lv[-1:] if m["dense"]}
    assert seen >= {"ell below 0", "csr below 0", "csr transpose", "dense last"}, seen


# ---- (a) the stored hierarchy ------------------------------------------------------------------------------------------------------------
def test_stored_hierarchy_is_what_the_comments_say(row):
    o = row
    levels, metas = o.cycle.levels, o.info["levels"]
    ratios = []
    for l, (lv, a, m) in enumerate(zip(levels, o.arrays, metas)):
        n = m["n"]
        r, c, v = lv.A
        # symmetric entry for entry; padding is col -1 / val 0; no diagonal entry among the couplings
        assert np.all((c >= 0) & (c < n)) and np.all(r != c), (o.tag, l)
        order, back = np.lexsort((c, r)), np.lexsort((r, c))
        assert np.array_equal(r[order], c[back]) and np.array_equal(c[order], r[back]) and np.array_equal(v[order], v[back]), (o.tag, l, "A != A^T")
        if m["layout"] == "ell":
            pad = a["col"] < 0
            assert np.all(a["col"][pad] == -1) and np.all(a["val"][pad] == 0) and pad.sum() + r.size == a["col"].size, (o.tag, l)
        assert np.all(lv.diag > 0), (o.tag, l)
        # a single-precision hierarchy is the rounded double one
        if o.info["f32"]:
            assert a["diag"].dtype == np.float32 and np.array_equal(a["diag"], a["diag64"].astype(np.float32)), (o.tag, l)
            assert np.array_equal(a["val"], a["val64"].astype(np.float32)), (o.tag, l)
        else:
            assert a["diag"].dtype == np.float64 and np.array_equal(a["diag"], a["diag64"]) and np.array_equal(a["val"], a["val64"])
        # smootherScale[l] lambda_max(D^-1 A_l)
        lam = mg_ref.lambda_max(lv)
        ratios.append(m["smootherScale"] * lam)
        if l + 1 == len(levels):
            break
        nc = metas[l + 1]["n"]
        d64, A64 = double_level(a, m)
        assert np.array_equal(A64[0], r) and np.array_equal(A64[1], c)
        if lv.P is not None:
            pr, pc, pv = lv.P
            tr, tc, tv = lv.PT
            assert np.all((pc >= 0) & (pc < nc)) and np.all((tc >= 0) & (tc < n)), (o.tag, l)
            # the stored P^T is the transpose of the stored P, value for value
            o1, o2 = np.lexsort((pr, pc)), np.lexsort((tc, tr))
            assert pr.size == tr.size and np.array_equal(pc[o1], tr[o2]) and np.array_equal(pr[o1], tc[o2]) and np.array_equal(pv[o1], tv[o2]), (o.tag, l, "P^T")
            pad = a["pCol"] < 0
            assert np.all(a["pVal"][pad] == 0) and np.all(a["pCol"][pad] == -1)
            Pd = np.zeros((n, nc))
            Pd[pr, pc] = pv
        else:
            agg = lv.agg
            assert np.all((agg >= 0) & (agg < nc)) and np.array_equal(np.sort(lv.aggItems), np.arange(n)), (o.tag, l, "each node once")
            assert lv.aggStart[0] == 0 and lv.aggStart[-1] == n and np.all(np.diff(lv.aggStart) > 0)
            owner = np.repeat(np.arange(nc), np.diff(lv.aggStart))
            assert np.array_equal(agg[lv.aggItems], owner), (o.tag, l, "aggStart / aggItems is not the inverse of agg")
            for I in (0, nc - 1):
                assert np.all(np.diff(lv.aggItems[lv.aggStart[I]:lv.aggStart[I + 1]]) > 0)
            Pd = np.zeros((n, nc))
            Pd[np.arange(n), agg] = 1.0
        # Galerkin: A_{l+1} = P^T A_l P in float64 from the decoded double arrays
        AP = d64[:, None] * Pd
        np.subtract.at(AP, A64[0], A64[2][:, None] * Pd[A64[1]])
        Ac = Pd.T @ AP
        stored = dense_double(o.arrays[l + 1], metas[l + 1])
        err = np.abs(Ac - stored).max() / np.abs(stored).max()
        if o.info["f32"] and lv.P is not None:
            # P exists in single precision only: each entry is off by <= 2^-24 relative, the product of two by <= 2 * 2^-24 (1 + 2^-24)
            absAP = np.abs(d64)[:, None] * np.abs(Pd)
            np.add.at(absAP, A64[0], np.abs(A64[2])[:, None] * np.abs(Pd)[A64[1]])
            bound = 2.0 ** -22 * (np.abs(Pd).T @ absAP).max() / np.abs(stored).max()
        else:
            bound = 1e-12
        print(f"PARITY {o.tag}: level {l + 1} |P^T A P - stored| / max|stored| = {err:.2e} (bound {bound:.1e})")
        assert err <= bound, (o.tag, l + 1, err, bound)
    last = levels[-1]
    if last.inverse is not None:
        A = dense_double(o.arrays[-1], metas[-1])
        defect = np.abs(last.inverse.astype(np.float64) @ A - np.eye(last.n)).max()
        print(f"PARITY {o.tag}: |inverse A - I| = {defect:.2e}")
        # double: 1e-9; single precision: n entries of a row, each rounded by 2^-24 relative
        bound = 1e-9 if not o.info["f32"] else 2.0 ** -24 * (np.abs(last.inverse.astype(np.float64)) @ np.abs(A)).max()
        assert defect <= bound, (o.tag, defect, bound)
    print(f"PARITY {o.tag}: smootherScale * lambda_max(D^-1 A) per level = {' '.join(f'{x:.3f}' for x in ratios)}")
    for l, x in enumerate(ratios):
        estimated = o.info["sa"] and l > 0
        assert estimated or metas[l]["smootherScale"] == 1.0, (o.tag, l)
        lo, hi = SCALE_BAND if estimated else LEVEL0_BAND
        assert lo <= x <= hi, (o.tag, l, ratios)


# smootherScale[l] * lambda_max(D^-1 A_l), lambda_max by power iteration here.  Levels without an estimate (level 0, every level of a plain
# aggregation) carry scale 1 for the Gershgorin bound 2: the product is lambda_max itself, measured 1.949 .. 2.000 on these meshes.  Estimated
# levels (smoothed aggregation, l > 0): the builder stores 2 / (1.1 x its own 30-step power-iteration estimate), i.e. 1.818 once that
# iteration has converged and more where it has not; measured over every row 1.817 .. 1.895 (profiles/mg_cycle_parity.txt), so [1.9, 2.2] does
# not hold there on a correct hierarchy and the band is the measured range widened by 5 %.  A scale of the wrong level or a scale left at 1
# gives 1.0 .. 1.2 or more than 2.
LEVEL0_BAND = (1.9, 2.2)
SCALE_BAND = (1.817 * 0.95, 1.895 * 1.05)


# ---- (b) one application ---------------------------------------------------------------------------------------------------------------------
def test_one_application_matches_the_replay(row):
    o = row
    for name, r in inputs(o):
        z = o.case.mg_apply(r)
        ref64 = o.cycle.apply(r, np.float64)
        scale = np.abs(ref64).max()
        dist = np.abs(z - ref64).max()
        assert np.isfinite(z).all() and scale > 0
        if o.info["f32"]:
            e32 = np.abs(o.cycle.apply(r, np.float32) - ref64).max()
            print(f"PARITY {o.tag}: {name:12s} e32 = {e32 / scale:.3e}  |z_dev - z_ref64| = {dist / scale:.3e}  ratio {dist / e32:.2f}  (relative to max|z_ref64|)")
            assert dist <= 4.0 * e32, (o.tag, name, dist / scale, e32 / scale, "\n" + localise(o, r))
        else:
            print(f"PARITY {o.tag}: {name:12s} |z_dev - z_ref64| = {dist / scale:.3e}  (relative to max|z_ref64|)")
            assert dist <= 1e-10 * scale, (o.tag, name, dist / scale, "\n" + localise(o, r))


def test_fused_tail_is_the_separate_passes(row):
    """mode 1 (mgSmoothLastKernel): z bit for bit that of the separate passes, the partial sums of r.z per block of 256 rows"""
    o = row
    if not o.info["fused"]:
        assert not o.info["f32"] or len(o.info["levels"]) < 2 or o.info["levels"][0]["layout"] != "ell", o.info
        with pytest.raises(q.QgdError) as ei:
            o.case.mg_apply(np.ones(o.n), tail=True)
        assert ei.value.code == L.ERR_INVALID
        return
    rows = o.info["partRows"]
    assert rows == 256
    for name, r in inputs(o):
        z0 = o.case.mg_apply(r)
        z1, part = o.case.mg_apply(r, tail=True)
        assert np.array_equal(z0, z1), (o.tag, name, np.abs(z0 - z1).max())
        assert np.array_equal(z1, z1.astype(np.float32).astype(np.float64))
        nb = (o.n + rows - 1) // rows
        assert part.size == nb
        terms = np.zeros(nb * rows); terms[:o.n] = r * z1
        terms = terms.reshape(nb, rows)
        want, mass = terms.sum(axis=1), np.abs(terms).sum(axis=1)
        # a sum of 256 terms in any order is off by rounding relative to the sum of the MAGNITUDES; relative to the sum itself no order of
        # summation keeps 1e-14 where a block cancels (z is dominated by a smooth mode, so r_i z_i changes sign with r_i): that figure is
        # printed, not asserted (measured up to 2e-14 on the hex rows, profiles/mg_cycle_parity.txt)
        rel_mass = (np.abs(part - want) / np.maximum(mass, 1e-300)).max()
        rel_sum = (np.abs(part - want) / np.maximum(np.abs(want), 1e-300)).max()
        print(f"PARITY {o.tag}: {name:12s} r.z partials: |part - sum| / sum|r_i z_i| = {rel_mass:.1e}   / |sum| = {rel_sum:.1e}   "
              f"cancellation sum|r_i z_i| / |sum| up to {(mass / np.maximum(np.abs(want), 1e-300)).max():.0f}")
        assert np.all(np.abs(part - want) <= 1e-14 * mass), (o.tag, name, rel_mass)
        assert abs(part.sum() - r @ z1) <= 1e-14 * mass.sum(), (o.tag, name)


# ---- (c) the operator CG needs -----------------------------------------------------------------------------------------------------------
def test_cycle_is_symmetric_on_random_pairs(row):
    o = row
    rng = np.random.default_rng(11)
    dev, rep = [], []
    for _ in range(3):
        x, y = rng.standard_normal((2, o.n))
        My, Mx = o.case.mg_apply(y), o.case.mg_apply(x)
        scale = np.linalg.norm(x) * np.linalg.norm(My)
        dev.append(abs(x @ My - y @ Mx) / scale)
        if o.info["f32"]:
            rep.append(abs(x @ o.cycle.apply(y, np.float32) - y @ o.cycle.apply(x, np.float32)) / scale)
    if o.info["f32"]:
        print(f"PARITY {o.tag}: |x.My - y.Mx| / (|x| |My|), three pairs: device {' '.join(f'{d:.2e}' for d in dev)}  replay32 {' '.join(f'{d:.2e}' for d in rep)}")
        assert max(dev) <= 4.0 * max(rep), (o.tag, dev, rep)
    else:
        print(f"PARITY {o.tag}: |x.My - y.Mx| / (|x| |My|), three pairs: device {' '.join(f'{d:.2e}' for d in dev)}")
        assert max(dev) <= 1e-10, (o.tag, dev)


def dense_operator(apply, n):
    M = np.zeros((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        M[:, j] = apply(e)
        e[j] = 0.0
    return M


@pytest.mark.parametrize("tag", ["double hex", "hex", "singular", "singular deep"])
def test_dense_operator_is_symmetric_positive(tag):
    """M column by column on the 960-cell mesh (960 applications; the one-level singular row has 880 cells)"""
    with observe(tag) as o:
        M = dense_operator(o.case.mg_apply, o.n)
        R64 = dense_operator(lambda e: o.cycle.apply(e, np.float64), o.n)
        A0 = dense_of(o.cycle.levels[0])
        top = np.abs(M).max()
        defect = np.abs(M - M.T).max() / top
        ev = np.linalg.eigvalsh(0.5 * (M + M.T))
        ev_ref = np.linalg.eigvalsh(0.5 * (R64 + R64.T))
        if o.info["f32"]:
            R32 = dense_operator(lambda e: o.cycle.apply(e, np.float32), o.n)
            defect32 = np.abs(R32 - R32.T).max() / np.abs(R32).max()
            print(f"PARITY {tag}: dense M, max|M - M^T| / max|M|: device {defect:.3e}  replay32 {defect32:.3e}  ratio {defect / defect32:.2f};"
                  f"  eigenvalues of (M + M^T)/2 in [{ev.min():.3e}, {ev.max():.3e}]")
            assert defect <= 4.0 * defect32, (tag, defect, defect32)
            # Weyl: the eigenvalues of the device operator lie within |M_dev - M_ref64|_2 of the replay's, itself allowed 4 x the replay32's distance
            slack = 4.0 * np.linalg.norm(0.5 * (R32 + R32.T) - 0.5 * (R64 + R64.T), 2)
        else:
            print(f"PARITY {tag}: dense M, max|M - M^T| / max|M|: device {defect:.3e};  eigenvalues of (M + M^T)/2 in [{ev.min():.3e}, {ev.max():.3e}]")
            assert defect <= 1e-10, (tag, defect)
            slack = 1e-10 * ev_ref.max()
        if o.singular:
            assert ev_ref.min() >= -1e-12 * ev_ref.max() and ev.min() >= ev_ref.min() - slack, (tag, ev.min(), ev_ref.min(), slack)
            return
        assert ev_ref.min() > 0 and ev.min() > 0 and ev.min() >= ev_ref.min() - slack, (tag, ev.min(), ev_ref.min(), slack)
        # the spectrum CG sees: condition number of M A_0 against the replayed cycle's, within 1 %
        k_dev, k_ref = (np.linalg.eigvals(X @ A0).real for X in (M, R64))
        kd, kr = k_dev.max() / k_dev.min(), k_ref.max() / k_ref.min()
        print(f"PARITY {tag}: kappa(M A_0) device {kd:.4f}  replay {kr:.4f}")
        assert k_dev.min() > 0 and abs(kd - kr) <= 0.01 * kr, (tag, kd, kr)


# ---- (d) the hooks are inert ----------------------------------------------------------------------------------------------------------------
def test_hooks_change_no_bit_of_a_run():
    mesh = MESHES["hex"]()
    res = {}
    for hooks in (False, True):
        dev = q.Device(mesh)
        with knobs(DEEP):
            c = qhdfoam.QHDFoamCase(dev, options(deltaT=1e-3, pTol=1e-10))
            cavity_bcs(c, mesh)
            c.set_fields(*initial(mesh))
        its = []
        for k in range(6):
            if hooks and k == 3:
                assert c.mg_info()["fused"]
                rng = np.random.default_rng(0)
                for _ in range(5):
                    r = rng.standard_normal(mesh.nCells)
                    z0 = c.mg_apply(r)
                    z1, _ = c.mg_apply(r, tail=True)
                    assert np.abs(z0).max() > 0 and np.array_equal(z0, z1)
                c.mg_level(0)
            c.step(1)
            its.append(c.info()["pIterations"])
        res[hooks] = {k: c.field(k) for k in ("U", "T", "p", "phi")}
        res[hooks]["its"] = its
        c.close(); dev.close()
    assert res[0]["its"] == res[1]["its"] and min(res[0]["its"]) >= 2, (res[0]["its"], res[1]["its"])
    for k in ("U", "T", "p", "phi"):
        assert np.isfinite(res[0][k]).all() and np.array_equal(res[0][k], res[1][k]), k


def test_entries_refuse_what_they_do_not_serve():
    mesh = q.PolyMesh.box(6, 5, 4)
    dev = q.Device(mesh)
    c = qhdfoam.QHDFoamCase(dev, options())
    cavity_bcs(c, mesh)
    for call in (c.mg_info, lambda: c.mg_level(0), lambda: c.mg_apply(np.ones(mesh.nCells))):
        with pytest.raises(q.QgdError) as ei:
            call()
        assert ei.value.code == L.ERR_INVALID
    c.close()
    c = qhdfoam.QHDFoamCase(dev, options(precond=0))
    cavity_bcs(c, mesh)
    c.set_fields(*initial(mesh))
    for call in (c.mg_info, lambda: c.mg_level(0), lambda: c.mg_apply(np.ones(mesh.nCells))):
        with pytest.raises(q.QgdError) as ei:
            call()
        assert ei.value.code == L.ERR_NOT_IMPLEMENTED
    c.close()
    # a shard (one k-slab of two, on this card): refused whether its hierarchy would span the ranks or stay local
    from qhd_shards import box_slabs
    sh = box_slabs(6, 5, 12, 2)[0]
    for env in ({}, {"QGD_MG_DIST": "0"}):
        sdev = q.Device(sh["mesh"])
        with knobs(env):
            c = qhdfoam.QHDFoamCase(sdev, options())
            cavity_bcs(c, sh["mesh"])
            n = sh["mesh"].nCells
            c.set_fields(np.zeros((n, 3)), np.full(n, 300.0), np.zeros(n))
        for call in (c.mg_info, lambda: c.mg_level(0), lambda: c.mg_apply(np.ones(n))):
            with pytest.raises(q.QgdError) as ei:
                call()
            assert ei.value.code == L.ERR_NOT_IMPLEMENTED
        c.close(); sdev.close()
    with knobs({"QGD_MG_PT_ELL_MIN": "-1"}):
        c = qhdfoam.QHDFoamCase(dev, options())
        cavity_bcs(c, mesh)
        with pytest.raises(q.QgdError, match="QGD_MG_PT_ELL_MIN"):
            c.set_fields(*initial(mesh))
        c.close()
    dev.close()
