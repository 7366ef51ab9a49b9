"""The pressure preconditioner of QHDFoam's CG, z = M r, restated in numpy (test infrastructure; no device code is called here).

One V-cycle of a (smoothed-)aggregation multigrid hierarchy, as DESIGN.md section 1 and the comments of qgd_poisson.hip describe it:

  level l < last, right-hand side b, iterate x from zero, D = diag(A_l), s_l = smootherScale[l] (2 / lambda_max(D^-1 A_l), 1 on level 0
  and on every level of a plain-aggregation hierarchy), n_l sweeps (nu0 on level 0, nu below):
    pre-smoothing    x_1 = cr[0] s_l D^-1 b;   x_{k+1} = (1 + cm[k]) x_k + cr[k] s_l D^-1 (b - A x_k) - cm[k] x_{k-1}   (x_0 = 0)
    residual         r = b - A x
    restriction      b_{l+1} = P^T r      (the STORED transpose; plain aggregation: the sum over each aggregate)
    coarse           e = cycle(l + 1, b_{l+1})
    correction       x += oc P e           (plain aggregation: x_i += oc e[agg_i])
    post-smoothing   the same n_l steps k = 0 .. n_l - 1, now from x (the step with cm[0] = 0 needs no previous iterate)
  damped Jacobi is cr[k] = omega, cm[k] = 0; QGD_MG_CHEB fills cr / cm with the Chebyshev recurrence.
  last level: x = inverse b (dense, row-major) or, without an inverse, coarseSweeps damped-Jacobi sweeps with omega s_l from zero.

A level is given by the arrays the device holds (QHDFoamCase.mg_level) and the parameters of QHDFoamCase.mg_info; `Level` decodes the two
storage layouts into (row, col, val) triples and applies them with np.bincount (float64) or np.add.at (float32, so that the sums are
rounded to single precision as they accumulate).  No dense matrix is formed except the stored inverse.  `dtype` selects the
precision of the whole replay: every vector, every coefficient and every scalar factor is rounded to it, as the cycle templates do."""
import numpy as np

STAGES = ("pre", "residual", "restricted", "coarse", "prolonged", "post")


# ---- the two storage layouts -----------------------------------------------------------------------------------------------------------
def decode_ell(start, col, val, n):
    """sliced ELL -> (row, col, val): 64 rows per slice, entry k of row i at (start[i >> 6] + k) * 64 + (i & 63); col < 0 is padding"""
    start, col, val = np.asarray(start), np.asarray(col), np.asarray(val)
    rows = np.arange(n, dtype=np.int64)
    width = (start[(rows >> 6) + 1] - start[rows >> 6]).astype(np.int64)
    wmax = int(width.max()) if n else 0
    k = np.arange(wmax, dtype=np.int64)[None, :]
    at = (start[rows >> 6].astype(np.int64)[:, None] + k) * 64 + (rows & 63)[:, None]
    ok = k < width[:, None]
    at = np.where(ok, at, 0)
    c = np.where(ok, col[at] if col.size else 0, -1)
    keep = c >= 0
    r = np.broadcast_to(rows[:, None], c.shape)
    return r[keep], c[keep].astype(np.int64), val[at][keep]


def decode_csr(start, col, val, n):
    start = np.asarray(start, dtype=np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(start[:n + 1]))
    m = int(start[n])
    return r, np.asarray(col[:m], dtype=np.int64), np.asarray(val[:m])


def encode_ell(n, row, col, val, dtype=np.float64):
    """(row, col, val) -> (start, col, val) as sliced ELL; the entries of a row keep their order; padding: col -1, val 0"""
    row, col, val = np.asarray(row, dtype=np.int64), np.asarray(col), np.asarray(val)
    ns = (n + 63) // 64
    deg = np.bincount(row, minlength=n) if n else np.zeros(0, dtype=np.int64)
    start = np.zeros(ns + 2, dtype=np.int32)
    for s in range(ns):
        start[s + 1] = start[s] + int(deg[s * 64:min(n, s * 64 + 64)].max())
    start[ns + 1] = start[ns]
    size = max(int(start[ns]) * 64, 1)
    oc, ov = np.full(size, -1, dtype=np.int32), np.zeros(size, dtype=dtype)
    order = np.argsort(row, kind="stable")
    first = np.concatenate(([0], np.cumsum(deg)))[:-1] if n else np.zeros(0, dtype=np.int64)
    k = np.arange(row.size) - first[row[order]]
    at = (start[row[order] >> 6].astype(np.int64) + k) * 64 + (row[order] & 63)
    oc[at], ov[at] = col[order], val[order]
    return start, oc, ov


def encode_csr(n, row, col, val, dtype=np.float64):
    row = np.asarray(row, dtype=np.int64)
    order = np.argsort(row, kind="stable")
    start = np.concatenate(([0], np.cumsum(np.bincount(row, minlength=n)))).astype(np.int32)
    if row.size == 0:       # the arrays are never empty: one unused element, as on the device
        return start, np.zeros(1, dtype=np.int32), np.zeros(1, dtype=dtype)
    return start, np.asarray(col)[order].astype(np.int32), np.asarray(val)[order].astype(dtype)


def apply_triples(n, row, col, val, x, dtype):
    """y_i = sum val x[col] over the triples of row i, accumulated in `dtype`"""
    prod = (val.astype(dtype) * x[col].astype(dtype)).astype(dtype)
    if np.dtype(dtype) == np.float64:
        return np.bincount(row, weights=prod, minlength=n).astype(np.float64) if row.size else np.zeros(n)
    y = np.zeros(n, dtype=dtype)
    np.add.at(y, row, prod)
    return y


class Level:
    """one level from the arrays of QHDFoamCase.mg_level (or hand-built ones with the same names) and its entry of mg_info()['levels']"""

    def __init__(self, arrays, meta, n_next=0):
        a = arrays
        self.n, self.meta, self.n_next = int(meta["n"]), dict(meta), int(n_next)
        self.scale = float(meta.get("smootherScale", 1.0))
        self.diag = np.asarray(a["diag"])
        dec = decode_csr if meta["layout"] == "csr" else decode_ell
        self.A = dec(a["start"], a["col"], a["val"], self.n)          # val = a_ij, A_ij = -a_ij (i != j)
        self.inverse = np.asarray(a["inverse"]).reshape(self.n, self.n) if "inverse" in a else None
        self.P = self.PT = self.agg = None
        if "pS" in a:
            self.P = decode_ell(a["pS"], a["pCol"], a["pVal"], self.n)
            self.PT = (decode_ell if meta.get("ptSliced") else decode_csr)(a["ptS"], a["ptCol"], a["ptVal"], self.n_next)
        elif "agg" in a:
            self.agg = np.asarray(a["agg"], dtype=np.int64)
            self.aggStart, self.aggItems = np.asarray(a["aggStart"], dtype=np.int64), np.asarray(a["aggItems"], dtype=np.int64)

    # A x, P^T r, P e in the precision `dt`
    def matvec(self, x, dt):
        off = apply_triples(self.n, *self.A, x, dt)
        return (self.diag.astype(dt) * x - off).astype(dt)

    def restrict(self, r, dt, with_stored_transpose=True):
        if self.P is not None:
            if with_stored_transpose:
                return apply_triples(self.n_next, *self.PT, r, dt)
            return apply_triples(self.n_next, self.P[1], self.P[0], self.P[2], r, dt)
        # plain aggregation: the members of aggregate I are aggItems[aggStart[I] : aggStart[I + 1]]
        owner = np.repeat(np.arange(self.n_next, dtype=np.int64), np.diff(self.aggStart))
        return apply_triples(self.n_next, owner, self.aggItems, np.ones(self.n, dtype=dt), r, dt)

    def prolong(self, e, dt):
        if self.P is not None:
            return apply_triples(self.n, *self.P, e, dt)
        return e[self.agg].astype(dt)


class Cycle:
    """z = M r from the levels and the parameters (the dict of QHDFoamCase.mg_info, or one with the same keys)"""

    def __init__(self, levels, info):
        self.levels, self.info = levels, info

    @classmethod
    def from_case_arrays(cls, info, arrays):
        sizes = [m["n"] for m in info["levels"]] + [0]
        return cls([Level(a, m, sizes[l + 1]) for l, (a, m) in enumerate(zip(arrays, info["levels"]))], info)

    def _step(self, lv, dt, w, b, x, prev, cx, cm):
        d = lv.diag.astype(dt)
        v = dt(cx) * x + dt(w) * (b - lv.matvec(x, dt)) / d
        if cm != 0.0 and prev is not None:
            v = v - dt(cm) * prev
        return v.astype(dt)

    def solve_level(self, l, b, dt, trace=None, exact_last=False, stored_transpose=True):
        p, lv = self.info, self.levels[l]
        dt = np.dtype(dt).type
        b = b.astype(dt)
        d = lv.diag.astype(dt)
        sc = lv.scale
        rec = (lambda stage, v: trace.setdefault(l, {}).__setitem__(stage, v.astype(np.float64))) if trace is not None else (lambda *a: None)
        if l + 1 == len(self.levels):
            if exact_last:     # the reference inverse: a float64 solve with the decoded matrix (for localising a mismatch)
                A = np.diag(lv.diag.astype(np.float64))
                np.subtract.at(A, (lv.A[0], lv.A[1]), lv.A[2].astype(np.float64))
                x = np.linalg.lstsq(A, b.astype(np.float64), rcond=None)[0].astype(dt)
            elif lv.inverse is not None:
                x = (lv.inverse.astype(dt) @ b).astype(dt)
            else:
                om = dt(p["omega"] * sc)
                x = (om * b / d).astype(dt)
                for _ in range(1, int(p["coarseSweeps"])):
                    x = (x + om * (b - lv.matvec(x, dt)) / d).astype(dt)
            rec("coarse", x)
            return x
        nu = int(p["nu0"]) if l == 0 else int(p["nu"])
        cr, cm = p["cr"], p["cm"]
        x = (dt(cr[0] * sc) * b / d).astype(dt)
        prev = None
        for s in range(1, nu):
            x, prev = self._step(lv, dt, cr[s] * sc, b, x, prev if s >= 2 else None, 1.0 + cm[s], cm[s] if s >= 2 else 0.0), x
        rec("pre", x)
        r = (b - lv.matvec(x, dt)).astype(dt)
        rec("residual", r)
        bc = lv.restrict(r, dt, stored_transpose)
        rec("restricted", bc)
        e = self.solve_level(l + 1, bc, dt, trace, exact_last, stored_transpose)
        x = (x + dt(p["oc"]) * lv.prolong(e, dt)).astype(dt)
        rec("prolonged", x)
        prev = None
        for s in range(nu):
            x, prev = self._step(lv, dt, cr[s] * sc, b, x, prev, 1.0 + cm[s], cm[s]), x
        rec("post", x)
        return x

    def apply(self, r, dtype=np.float64, **kw):
        """z = M r; the vector enters and leaves in float64 (the CG's), the cycle runs in `dtype`"""
        r = np.asarray(r, dtype=np.float64)
        return self.solve_level(0, r.astype(dtype), dtype, **kw).astype(np.float64)

    def matrix(self, dtype=np.float64):
        n = self.levels[0].n
        M = np.zeros((n, n))
        e = np.zeros(n)
        for j in range(n):
            e[j] = 1.0
            M[:, j] = self.apply(e, dtype)
            e[j] = 0.0
        return M


def lambda_max(level, tol=1e-6, max_it=20000, seed=0):
    """largest eigenvalue of D^-1 A by power iteration on the symmetric D^-1/2 A D^-1/2 (Rayleigh quotients, to `tol` relative)"""
    dh = 1.0 / np.sqrt(level.diag.astype(np.float64))
    x = np.random.default_rng(seed).standard_normal(level.n)
    lam = 0.0
    for it in range(max_it):
        x /= np.linalg.norm(x)
        y = dh * level.matvec(dh * x, np.float64)
        new = float(x @ y)
        if it > 10 and abs(new - lam) <= 0.01 * tol * abs(new):
            # the Rayleigh quotient converges twice as fast as the vector: check the residual too
            if np.linalg.norm(y - new * x) <= np.sqrt(tol) * abs(new):
                return new
        lam, x = new, y
    return lam
