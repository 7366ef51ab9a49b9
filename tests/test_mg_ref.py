"""CPU: the numpy replay of the pressure multigrid cycle (tests/mg_ref.py) checked on hierarchies built by hand.

1-D and 2-D Poisson matrices, textbook aggregates of 3 (3 x 3 in 2-D), the tentative prolongator smoothed by one Jacobi step,
P = (I - 4 / (3 lambda_max) D^-1 A) T, and the Galerkin operator A_c = P^T A P formed densely in numpy here; the arrays are then stored in the two device layouts
(sliced ELL, CSR rows) with the names QHDFoamCase.mg_level returns, so the replay reads them exactly as it reads a device hierarchy.
What must hold for any correct restatement of the cycle: it is a symmetric positive definite operator, as a stationary iteration
it contracts the error of A x = b, with the smoother switched off and an exact coarse solve it is oc P A_c^-1 P^T, with damped Jacobi its
error propagator is the textbook two-grid product, and the two layouts round-trip at ragged slices and at the widths around the kernels'
8-entry batch."""
import numpy as np
import pytest

import mg_ref


def poisson_1d(n):
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def poisson_2d(nx, ny):
    return np.kron(np.eye(ny), poisson_1d(nx)) + np.kron(poisson_1d(ny), np.eye(nx))


def aggregates_1d(n):
    return np.arange(n) // 3


def aggregates_2d(nx, ny):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    return ((j // 3) * ((nx + 2) // 3) + i // 3).ravel()


def chebyshev(ratio, lmax=2.0, omega=0.8):
    """cr / cm of the smoother's steps: Chebyshev polynomial of D^-1 A on [lmax / ratio, lmax]; ratio 0: damped Jacobi"""
    cr, cm = np.full(8, omega), np.zeros(8)
    if ratio > 1:
        theta, delta = 0.5 * (lmax + lmax / ratio), 0.5 * (lmax - lmax / ratio)
        sigma = theta / delta
        rho = 1.0 / sigma
        cr[0] = 1.0 / theta
        for k in range(1, 8):
            new = 1.0 / (2.0 * sigma - rho)
            cm[k], cr[k] = new * rho, 2.0 * new / delta
            rho = new
    return cr, cm


def triples_of(M):
    r, c = np.nonzero(M)
    return r, c, M[r, c]


def store_level(A, layout, P=None, pt_sliced=False, agg=None, inverse=False, scale=1.0, dtype=np.float64):
    """dense A (and P or agg) -> (arrays, meta) in the device's naming and layouts; off-diagonal entries are stored as a_ij = -A_ij"""
    n = A.shape[0]
    off = -(A - np.diag(np.diag(A)))
    enc = mg_ref.encode_csr if layout == "csr" else mg_ref.encode_ell
    start, col, val = enc(n, *triples_of(off), dtype=dtype)
    a = dict(diag=np.diag(A).astype(dtype), start=start, col=col, val=val)
    meta = dict(n=n, layout=layout, dense=inverse, smoothed=P is not None, ptSliced=pt_sliced, smootherScale=scale)
    if inverse:
        a["inverse"] = np.linalg.inv(A).astype(dtype).ravel()
    if P is not None:
        a["pS"], a["pCol"], a["pVal"] = mg_ref.encode_ell(n, *triples_of(P), dtype=dtype)
        a["ptS"], a["ptCol"], a["ptVal"] = (mg_ref.encode_ell if pt_sliced else mg_ref.encode_csr)(P.shape[1], *triples_of(P.T.copy()), dtype=dtype)
    elif agg is not None:
        a["agg"] = agg.astype(np.int32)
        a["aggItems"] = np.argsort(agg, kind="stable").astype(np.int32)
        a["aggStart"] = np.concatenate(([0], np.cumsum(np.bincount(agg)))).astype(np.int32)
    return a, meta


def build(A0, aggs, smoothed=True, layouts=None, last="dense", ratio=0.0, nu=2, nu0=None, oc=1.0, coarse_sweeps=40, pt_sliced=(), dtype=np.float64):
    """hierarchy A0 -> A1 -> ... over the aggregate maps `aggs`; returns (Cycle, dense [A_l], dense [P_l])"""
    As, Ps, arrays, metas = [A0], [], [], []
    for agg in aggs:
        A = As[-1]
        T = np.zeros((A.shape[0], agg.max() + 1))
        T[np.arange(A.shape[0]), agg] = 1.0
        d = np.diag(A)
        lmax = np.linalg.eigvalsh(A / np.sqrt(np.outer(d, d))).max()
        P = (np.eye(A.shape[0]) - (4.0 / 3.0) / lmax * A / d[:, None]) @ T if smoothed else T
        Ps.append(P)
        As.append(P.T @ A @ P)
    layouts = layouts or ["ell"] + ["csr"] * len(aggs)
    for l, A in enumerate(As):
        d = np.diag(A)
        scale = 1.0 if (l == 0 or not smoothed) else 2.0 / np.linalg.eigvalsh(A / np.sqrt(np.outer(d, d))).max()
        is_last = l == len(aggs)
        a, m = store_level(A, layouts[l], P=Ps[l] if smoothed and not is_last else None, pt_sliced=l in pt_sliced,
                           agg=None if smoothed or is_last else aggs[l], inverse=is_last and last == "dense", scale=scale, dtype=dtype)
        arrays.append(a); metas.append(m)
    cr, cm = chebyshev(ratio)
    info = dict(levels=metas, f32=dtype == np.float32, sa=smoothed, omega=0.8, oc=oc, nu=nu, nu0=nu0 or nu, coarseSweeps=coarse_sweeps, cr=cr, cm=cm)
    return mg_ref.Cycle.from_case_arrays(info, arrays), As, Ps


def hierarchy_1d(n=200, **kw):
    a1 = aggregates_1d(n)
    a2 = aggregates_1d(a1.max() + 1)
    return build(poisson_1d(n), [a1, a2], **kw)


def hierarchy_2d(nx=17, ny=13, **kw):
    return build(poisson_2d(nx, ny), [aggregates_2d(nx, ny)], **kw)


CONFIGS = {
    "1d jacobi": lambda: hierarchy_1d(),
    "1d sliced transpose, ell below": lambda: hierarchy_1d(layouts=["ell", "ell", "csr"], pt_sliced=(0, 1)),
    "1d chebyshev nu=3": lambda: hierarchy_1d(ratio=10.0, nu=3),
    "1d nu0=1": lambda: hierarchy_1d(nu0=1),
    "1d sweeps on the last level": lambda: hierarchy_1d(last="sweeps", layouts=["ell", "csr", "ell"]),
    "1d plain aggregation, oc=1.8": lambda: hierarchy_1d(smoothed=False, oc=1.8, layouts=["ell", "ell", "ell"]),
    "2d jacobi": lambda: hierarchy_2d(),
    "2d chebyshev nu=4, nu0=2": lambda: hierarchy_2d(ratio=6.0, nu=4, nu0=2),
}


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def dense_cycle(request):
    cyc, As, Ps = CONFIGS[request.param]()
    return request.param, cyc, As, Ps, cyc.matrix()


def test_replayed_cycle_is_symmetric(dense_cycle):
    tag, cyc, As, _, M = dense_cycle
    normM = np.linalg.norm(M, 2)
    rng = np.random.default_rng(1)
    for _ in range(5):
        x, y = rng.standard_normal((2, M.shape[0]))
        d = abs(x @ cyc.apply(y) - y @ cyc.apply(x))
        assert d <= 1e-13 * np.linalg.norm(x) * normM * np.linalg.norm(y), (tag, d)
    assert np.abs(M - M.T).max() <= 1e-13 * normM, tag


def test_replayed_cycle_is_positive_definite(dense_cycle):
    tag, _, _, _, M = dense_cycle
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    assert ev.min() > 1e-6 * ev.max(), (tag, ev.min(), ev.max())


def test_replayed_cycle_contracts_the_error_as_a_stationary_iteration(dense_cycle):
    tag, cyc, As, _, M = dense_cycle
    A = As[0]
    ev = np.linalg.eigvals(M @ A).real
    if "oc=1.8" in tag:
        # the over-weighted plain aggregation is meant for CG only: as an iteration it need not contract, its spectrum stays positive
        assert ev.min() > 0, (tag, ev.min())
        return
    assert 0 < ev.min() and ev.max() < 2, (tag, ev.min(), ev.max())
    rng = np.random.default_rng(2)
    xs = rng.standard_normal(A.shape[0])
    b = A @ xs
    x = np.zeros_like(xs)
    err = [np.sqrt((x - xs) @ A @ (x - xs))]
    for _ in range(12):
        x = x + cyc.apply(b - A @ x)
        err.append(np.sqrt((x - xs) @ A @ (x - xs)))
    ratios = np.array(err[1:]) / np.array(err[:-1])
    assert ratios.max() < 1.0 and err[-1] < 1e-3 * err[0], (tag, ratios)


@pytest.mark.parametrize("dims", [1, 2])
def test_without_smoothing_the_cycle_is_the_coarse_correction(dims):
    """cr = 0 switches every smoothing step off (x stays 0 before, unchanged after): M = oc P A_c^-1 P^T to rounding"""
    cyc, As, Ps = hierarchy_2d(oc=1.3) if dims == 2 else build(poisson_1d(100), [aggregates_1d(100)], oc=1.3)
    cyc.info["cr"] = np.zeros(8)
    want = 1.3 * Ps[0] @ np.linalg.inv(As[1]) @ Ps[0].T
    got = cyc.matrix()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("dims", [1, 2])
def test_damped_jacobi_cycle_has_the_textbook_error_propagator(dims):
    """I - M A = S^nu (I - P A_c^-1 P^T A) S^nu with S = I - omega D^-1 A, formed densely here; three levels in 1-D (the coarse solve is
    itself a cycle, with S_1 = I - omega s_1 D_1^-1 A_1)"""
    cyc, As, Ps = hierarchy_1d(n=120) if dims == 1 else hierarchy_2d()
    om, nu = 0.8, 2

    def dense_M(l):
        A = As[l]
        if l + 1 == len(As):
            return np.linalg.inv(A)
        S = np.eye(A.shape[0]) - om * cyc.levels[l].scale * A / np.diag(A)[:, None]
        Sn = np.linalg.matrix_power(S, nu)
        E = Sn @ (np.eye(A.shape[0]) - Ps[l] @ dense_M(l + 1) @ Ps[l].T @ A) @ Sn
        return (np.eye(A.shape[0]) - E) @ np.linalg.inv(A)

    want = dense_M(0)
    assert np.abs(cyc.matrix() - want).max() <= 1e-11 * np.abs(want).max()


def test_single_precision_replay_is_rounded_to_single_precision():
    c64, _, _ = hierarchy_1d()
    c32, _, _ = hierarchy_1d(dtype=np.float32)
    r = np.random.default_rng(3).standard_normal(200)
    z64, z32 = c64.apply(r), c32.apply(r, np.float32)
    rel = np.abs(z32 - z64).max() / np.abs(z64).max()
    assert 1e-9 < rel < 1e-4, rel
    assert z32.dtype == np.float64 and np.array_equal(z32, z32.astype(np.float32).astype(np.float64))
    tr = {}
    c64.apply(r, trace=tr)
    assert sorted(tr) == [0, 1, 2] and set(tr[0]) == set(mg_ref.STAGES) - {"coarse"} and set(tr[2]) == {"coarse"}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 200])       # last slice of 1 row (65) and of 63 rows (63, 127)
@pytest.mark.parametrize("width", [1, 7, 8, 9, 17])
def test_layouts_round_trip(n, width):
    rng = np.random.default_rng(100 * n + width)
    deg = rng.integers(0, width + 1, n)
    deg[rng.integers(n)] = width
    row = np.repeat(np.arange(n), deg)
    col = rng.integers(0, max(n, 2), row.size)
    val = rng.standard_normal(row.size)
    # sliced ELL: the documented index formula, entry by entry, and padding everywhere else
    start, c, v = mg_ref.encode_ell(n, row, col, val)
    assert start.size == (n + 63) // 64 + 2 and c.size == v.size == max(64 * start[-1], 1)
    seen = np.zeros(c.size, dtype=bool)
    k = 0
    for e in range(row.size):
        i = row[e]
        k = k + 1 if e and row[e - 1] == i else 0
        at = (start[i >> 6] + k) * 64 + (i & 63)
        assert c[at] == col[e] and v[at] == val[e] and k < start[(i >> 6) + 1] - start[i >> 6]
        seen[at] = True
    assert np.all(c[~seen] == -1) and np.all(v[~seen] == 0.0)
    for s in range((n + 63) // 64):
        assert start[s + 1] - start[s] == deg[s * 64:s * 64 + 64].max()
    r2, c2, v2 = mg_ref.decode_ell(start, c, v, n)
    assert np.array_equal(r2, row) and np.array_equal(c2, col) and np.array_equal(v2, val)
    # CSR rows
    start, c, v = mg_ref.encode_csr(n, row, col, val)
    assert np.array_equal(np.diff(start), deg)
    r2, c2, v2 = mg_ref.decode_csr(start, c, v, n)
    assert np.array_equal(r2, row) and np.array_equal(c2, col) and np.array_equal(v2, val)
    # and both give the same product, in both precisions
    x = rng.standard_normal(max(n, 2))
    want = np.zeros(n)
    np.add.at(want, row, val * x[col])
    assert np.allclose(mg_ref.apply_triples(n, row, col, val, x, np.float64), want, rtol=0, atol=1e-13 * max(1.0, np.abs(want).max()))
    y32 = mg_ref.apply_triples(n, row, col, val.astype(np.float32), x.astype(np.float32), np.float32)
    assert y32.dtype == np.float32 and np.allclose(y32, want, rtol=0, atol=2e-6 * width * max(1.0, np.abs(val).max() * np.abs(x).max()))


def test_lambda_max_by_power_iteration():
    cyc, As, _ = hierarchy_2d()
    for lv, A in zip(cyc.levels, As):
        d = np.diag(A)
        want = np.linalg.eigvalsh(A / np.sqrt(np.outer(d, d))).max()
        assert abs(mg_ref.lambda_max(lv) - want) <= 1e-6 * want


@pytest.mark.parametrize("layout", ["ell", "csr"])
def test_level_without_couplings(layout):
    """a diagonal level stores one padding element (col -1 / 0, val 0) and no entry: the replay is D^-1-like and finite"""
    n = 70
    d = np.linspace(1.0, 2.0, n)
    a, m = store_level(np.diag(d), layout, inverse=False)
    assert a["col"].size == a["val"].size == 1 and a["val"][0] == 0.0
    info = dict(levels=[m], f32=False, sa=True, omega=0.8, oc=1.0, nu=2, nu0=2, coarseSweeps=40, cr=np.full(8, 0.8), cm=np.zeros(8))
    cyc = mg_ref.Cycle.from_case_arrays(info, [a])
    assert cyc.levels[0].A[0].size == 0
    r = np.random.default_rng(5).standard_normal(n)
    assert np.allclose(cyc.apply(r), (1.0 - 0.2 ** 40) * r / d, rtol=1e-13, atol=0)
